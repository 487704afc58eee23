/* somhip_ng_dense.h -- dense batch neural gas (K10d) on the MI355X SOM/LVQ engine: the part of the C ABI of libsomhip.so that
 * trains a codebook with neural gas over every rank.  include/somhip.h includes this file behind its own declarations (the
 * handles, the error convention, somhip_ng_params and somhip_last_error are there), so a program includes somhip.h alone.
 * The ctypes mirror is som_lvq_pak_amd/_lib.py NG_DENSE_SIGNATURES; tests/test_ngas_dense.py holds this header to the
 * checks tests/test_build.py makes of somhip.h: every declaration exported and mirrored. */
#ifndef SOMHIP_NG_DENSE_H
#define SOMHIP_NG_DENSE_H

#include "somhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense batch neural gas (K10d; no reference function) ---------------------------
 * Batch neural gas (somhip_ng_train, K10) without its truncation: every sample feeds EVERY unit, with the weight
 * exp(-rank / lambda) of the unit's rank among all units.  somhip_ng_train stops at the SOMHIP_KNN_MAX = 256 nearest units
 * of a sample; this form is for the codebooks beyond that, and for the early epochs, where lambda is large.
 * One call runs epochs t = start_epoch .. start_epoch + count - 1 of a run of T = epochs epochs over data rows
 * (first + s) % n_rows, s = 0 .. n-1, on a codebook of `units` <= SOMHIP_NG_DENSE_MAX rows.  Per epoch:
 *   1. in double on the host: lambda_t exactly as somhip_ng_train forms it; w[r] = exp(-(double)r / lambda_t) for every
 *      r < units.  No rule drops a rank and nothing caps their number; a weight that underflows is +0.0.  p->ranks must be 0
 *   2. d[s][j] for every sample and every row j: find_winner_euc's squared distance (fp32: sub, mul, add in dimension
 *      order from +0.0f, three roundings)
 *   3. rank[s][j] = the number of rows that come before row j in the order (distance ascending, the later row first among
 *      equal distances) -- find_winner_knn's order, what somhip_find_winners(..., SOMHIP_TIE_KNN) gives; Q[s][j] =
 *      w[rank[s][j]].  A row whose distance is not below FLT_MAX is ranked behind all others by the bits of its
 *      distance, and its Q is +0.0
 *   4. [S | W] = Q^T x [X | 1]: S[j][k] = sum_s Q[s][j] * (double)x_s[k], W[j] = sum_s Q[s][j], formed by
 *      v_mfma_f64_16x16x4_f64 as batch RSLVQ's step 4 (somhip_rslvq.h) forms [G | c]: the samples in data order, four
 *      consecutive samples inside one instruction, instruction after instruction into one accumulator.  The order is a
 *      function of (n, units, dim) alone -- the chunks the run is cut into do not change a bit -- and no floating-point
 *      atomics are used
 *   5. m_j[k] = (float)(S[j][k] / W[j]) where W[j] > 0 (somhip_ng_train's step 4); a row whose weights all underflowed, or
 *      that no sample has a distance below FLT_MAX to, keeps its bits
 * qerror_out (host, [count], or NULL): per epoch find_qerror's float sum over the rank-0 distances in data order -- the
 * quantization error of the codebook the epoch started from.
 * This is a second definition, not another route to somhip_ng_train's bits: step 4 adds four samples a step with fused
 * multiply-adds, where somhip_ng_train runs one multiply-then-add chain per unit.  The two agree only within the rounding
 * bound of the sums -- also on codebooks of at most 256 rows, where neither truncates.
 * Refused, with a message that names the entry point, before anything is launched and with the rows untouched:
 * everything somhip_ng_train refuses (data with x components, sharded codebooks, a dimension mismatch, n <= 0, n >= 2^32,
 * first < 0, epochs < 1, lambda0 not > 0, lambda_end not in (0, lambda0], epochs outside [0, epochs)), ranks != 0, and a
 * codebook of more than SOMHIP_NG_DENSE_MAX rows. */
#define SOMHIP_NG_DENSE_MAX 4096   /* one sample's 64-bit keys (32 KB) sort in one workgroup's LDS, several workgroups a CU */
int  somhip_ng_train_dense(somhip_codebook *cb, somhip_dataset *ds, const somhip_ng_params *p, float *qerror_out /*[count] or NULL*/);
/* The stages somhip_ng_train_dense is made of, each on its own.
 * _schedule: step 1 of epoch t for a codebook of `units` rows, on the host (no GPU): *lambda and weights[units].
 * _ranks: steps 2 and 3 to the host, rank_out / dist_out [n][units]: per sample and unit j the unit's rank and squared
 * distance.
 * _sums: steps 2-4 with w[r] = exp(-(double)r / lambda): sums [units][dim], wsum [units] to the host.  The run is walked
 * in chunks of `chunk` samples (0: the engine's own, batch RSLVQ's rule; else a multiple of 64 up to 4096); the chunks after
 * the first continue the accumulators, so every chunk length leaves the same bits.  somhip_debug_ng_update (somhip.h)
 * is step 5 on such sums. */
int  somhip_debug_ng_dense_schedule(const somhip_ng_params *p, int64_t units, int64_t t, double *lambda, double *weights /*[units]*/);
int  somhip_debug_ng_dense_ranks(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int32_t *rank_out, float *dist_out);
int  somhip_debug_ng_dense_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, double lambda, int64_t chunk,
                                double *sums, double *wsum);
/* HIP-event totals of its stages since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count, and outside somhip_timing_select's mask: timed whenever timing is on): [0] the distances (the
 * sample tiles and the distance kernel, one span per chunk), [1] the ranking kernel, [2] the sums.  The update counts
 * under somhip_ng_timing's [2]. */
int  somhip_ng_dense_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]);

#ifdef __cplusplus
}
#endif
#endif /* SOMHIP_NG_DENSE_H */
