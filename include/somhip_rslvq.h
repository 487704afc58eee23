/* somhip_rslvq.h -- batch Robust Soft LVQ (K13) on the MI355X SOM/LVQ engine: the part of the C ABI of libsomhip.so that
 * trains and evaluates the probabilistic member of the LVQ family.  include/somhip.h includes this file behind its own
 * declarations (the handles, the error convention and somhip_last_error are there), so a program includes somhip.h alone.
 * The ctypes mirror is som_lvq_pak_amd/_lib.py RSLVQ_SIGNATURES; tests/test_rslvq_abi.py holds this header to the checks
 * tests/test_build.py and tests/test_prepared_state.py make of somhip.h: every declaration exported and mirrored, every
 * entry point that takes a codebook it may write to checked against the codebook's prepared copies. */
#ifndef SOMHIP_RSLVQ_H
#define SOMHIP_RSLVQ_H

#include "somhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batch Robust Soft LVQ (K13; no reference function) -----------------------------
 * Seo and Obermayer's RSLVQ as full-batch gradient steps: the rows are the centres of a Gaussian mixture of one width,
 * E = mean_s -log P(y_s | x_s), and every sample moves every row in proportion to a posterior.  No winner, no window
 * rule; the same bits on every run.
 * One call runs epochs t = start_epoch .. start_epoch + count - 1 of a run of T = epochs epochs over data rows
 * (first + s) % n_rows, s = 0 .. n-1, against a labelled codebook.  Per epoch:
 *   1. alpha_t = alpha * (float)(T - t) / (float)T, in float (batch GLVQ's step 1)
 *   2. d[s][j] for every sample and every row j: find_winner_euc's squared distance (fp32: sub, mul, add in dimension
 *      order from +0.0f, three roundings)
 *   3. per sample in fp64, every operation one rounding in the order written: two_s = 2.0 * (double)sigma2,
 *      g_j = -(double)d_j / two_s; m_all = max_j g_j, m_own = the maximum over the rows whose label is the sample's;
 *      Z_all = ONE chain of additions from +0.0 in row order of exp(g_j - m_all); Z_own = the same chain over the
 *      own-label rows of exp(g_j - m_own); P_j = exp(g_j - m_all) / Z_all; q[s][j] = exp(g_j - m_own) / Z_own - P_j on
 *      own-label rows and -P_j on the others; cost_s = (m_all + log(Z_all)) - (m_own + log(Z_own)), which is
 *      -log P(y | x); pown_s = exp(-cost_s).  The sample counts as correct when the smallest key (d_j, j) among the
 *      own-label rows is smaller than the smallest among the others (batch GLVQ's rule)
 *   4. per row j: G[j][k] = sum_s q[s][j] * (double)x_s[k] and c[j] = sum_s q[s][j], formed as [G | c] = Q^T x [X | 1]
 *      by v_mfma_f64_16x16x4_f64: the samples in data order, four consecutive samples (4 i .. 4 i + 3 of the run) inside
 *      one instruction, instruction after instruction into one accumulator.  The order is a function of (n, rows, dim)
 *      alone -- the chunks the run is cut into do not change a bit -- and no floating-point atomics are used
 *   5. with W = (double)w_j[k] and a = (double)alpha_t / ((double)sigma2 * (double)n):
 *      w_j[k] = (float)(W + a * (G[j][k] - c[j] * W)); every row is stepped
 * cost_out (host, [count], or NULL): per epoch (the fp64 chain over cost_s in data order, formed on the host) / n;
 * correct_out (host, [count], or NULL): the number of correct samples.  Both describe the codebook the epoch started from.
 * alpha has the unit of a squared distance: the gradient of E carries 1 / sigma2, and the step is alpha_t / sigma2 times
 * a mean of q (x - w).
 * Refused, with a message that names the entry point, before anything is launched and with the codebook untouched:
 * everything somhip_glvq_train refuses (labels missing, x components, a data label no row carries, one class only, a
 * sharded codebook, the n, first and epoch ranges, alpha negative or NaN), and sigma2 not finite or <= 0. */
typedef struct somhip_rslvq_params {
  int64_t epochs;        /* T */
  int64_t start_epoch, count;
  int64_t first, n;      /* the data rows of every epoch */
  float   alpha;         /* the rate the run starts from */
  float   sigma2;        /* the squared width of every component of the mixture */
} somhip_rslvq_params;
int  somhip_rslvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_rslvq_params *p, double *cost_out /*[count] or NULL*/,
                        int64_t *correct_out /*[count] or NULL*/);
/* Steps 2 and 3 over a run, what evaluating a trained model needs: *cost and *correct as an epoch of _train reports them,
 * pown ([n], or NULL) = P(y | x) per sample.  It trains nothing and leaves the rows untouched. */
int  somhip_rslvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigma2, double *cost,
                         int64_t *correct, double *pown /*[n] or NULL*/);
/* The stages somhip_rslvq_train is made of, each on its own.  The run is walked in chunks of samples; _chunk: the chunk
 * every public entry takes for a codebook of n_rows rows -- min(4096, the largest multiple of 64 whose coefficients fit
 * 256 MiB), 64 at least -- and ld = 64 * ceil(n_rows / 64), the leading dimension of q (host arithmetic, no GPU).  The
 * stage entries take a chunk of their own: 0 for that rule, or a multiple of 64 up to 4096.
 * _posterior: steps 2 and 3 to the host: q_out [n][ld] with zeros in the columns behind the last row, cost_s, pown [n],
 * correct_s [n] (1 or 0).
 * _sums: step 4 on a caller's q_in [n][ld] (the columns behind the last row are not read into any result): G [n_rows][dim],
 * c [n_rows].
 * _update: step 5 on host-supplied G and c; it writes the codebook. */
int  somhip_debug_rslvq_chunk(int64_t n_rows, int64_t *chunk, int64_t *ld);
int  somhip_debug_rslvq_posterior(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigma2, int64_t chunk,
                                  double *q_out, double *cost_s, int32_t *correct_s, double *pown);
int  somhip_debug_rslvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int64_t chunk, const double *q_in,
                             double *G, double *c);
int  somhip_debug_rslvq_update(somhip_codebook *cb, float alpha_t, float sigma2, int64_t n, const double *G, const double *c);
/* HIP-event totals of its stages since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count, and outside somhip_timing_select's mask: timed whenever timing is on): [0] the distances (the
 * sample tiles and the distance kernel, one span per chunk), [1] the posteriors, [2] the sums, [3] the update */
int  somhip_rslvq_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]);

#ifdef __cplusplus
}
#endif
#endif /* SOMHIP_RSLVQ_H */
