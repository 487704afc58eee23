/* somhip_batchmap_missing.h -- the batch map (K8) over data with missing values (K8m): the part of the C ABI of libsomhip.so
 * that trains a map by Kohonen's batch rule where a sample may leave components out.  include/somhip.h includes this file
 * behind its own declarations (the handles, somhip_batchmap_params and the error convention are there), so a program
 * includes somhip.h alone.  The ctypes mirror is som_lvq_pak_amd/_lib.py BATCHMAP_MISSING_SIGNATURES;
 * tests/test_batchmap_missing.py holds this header to the checks tests/test_build.py makes of somhip.h: every declaration
 * exported and mirrored. */
#ifndef SOMHIP_BATCHMAP_MISSING_H
#define SOMHIP_BATCHMAP_MISSING_H

#include "somhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the batch map over data with missing values (K8m; no reference function) ------
 * Kohonen's own formulation for incomplete samples: a sample is matched over the components it has, and a model
 * vector's component becomes the weighted mean of the samples that know that component.  somhip_som_batchmap_missing has
 * the parameters, the epoch window and the radius schedule of somhip_som_batchmap, and takes data sets with or without a
 * mask.  Per epoch t:
 *   1. r_t as in somhip_som_batchmap.
 *   2. c(s) = find_winner_euc of sample s under the sample's mask (lvq_pak.c:179-186: only the sample's mask counts), the
 *      lowest index among equal distances (SOMHIP_TIE_FIRST).  A sample with every component masked has no winner: it
 *      feeds no sum and no count, and the qerror chain skips it as find_qerror does (som_rout.c:712).
 *   3. S[j][k] = ONE chain of fp64 additions from +0.0, in data order, of (double)x_s[k] over the samples with c(s) = j
 *      whose component k is known.  A masked component is skipped by a select: what is stored there never reaches a
 *      result, a NaN included.  C[j][k] = the number of those samples, an exact integer held as a double.
 *   4. h(i, j) as in somhip_som_batchmap.
 *   5. N[i][k] = sum_j h(i,j) S[j][k], D[i][k] = sum_j h(i,j) C[j][k] in fp64 (v_mfma_f64_16x16x4_f64, the additions over j in
 *      the order of somhip_som_batchmap's combine); m_i[k] = (float)(N[i][k] / D[i][k]) where D[i][k] > 0.  A COMPONENT
 *      with D[i][k] == 0 keeps its bits -- per component, not per row.
 * On data without masks (or with a mask of zeros) C[j][k] = hits[j] for every k, every D[i][k] is formed by the operations
 * that form somhip_som_batchmap's D[i], and the call leaves the bits of somhip_som_batchmap: rows and qerror_out.
 * Refused, with a message that names the entry point, before anything is launched and with the codebook untouched: what
 * somhip_som_batchmap refuses, but for data with x components.  (n < 2^32 stays: the lists are 32-bit.) */
int  somhip_som_batchmap_missing(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p,
                                 float *qerror_out /*[count] or NULL*/);
/* The two stages on their own.  _sums: steps 2-3 -- sums[n_rows of the codebook][dim] and counts[n_rows][dim] to the host.
 * _combine: steps 4-5 at radius r (>= 0) on host-supplied sums and counts; it writes the codebook. */
int  somhip_debug_batchmap_missing_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, double *sums,
                                        double *counts);
int  somhip_debug_batchmap_missing_combine(somhip_codebook *cb, float r, const double *sums, const double *counts);
/* The same epoch over data in pieces: the five calls of somhip_batchmap_begin / _accumulate / _finish / _end / _state with
 * their semantics, on a state of this form -- [S | C] as n_rows x 2 dim doubles, row j holding S[j][0 .. dim) and behind
 * it C[j][0 .. dim), all +0.0 when opened, then the same tail of 16 bytes {float q; uint32 unused; uint64 samples}.
 * A codebook holds at most ONE open batch-map accumulation, of either form: _begin of one form gives up a state of the
 * other.  somhip_batchmap_accumulate / _finish / _state on a state of this form, and these calls on a state of the plain
 * form, are refused by name, rows and state untouched.  Every other refusal, and what closes the state, is as there.  The
 * launches count under the three ids of somhip_batchmap_timing. */
int  somhip_batchmap_missing_begin(somhip_codebook *cb);
int  somhip_batchmap_missing_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int want_qerror);
int  somhip_batchmap_missing_finish(somhip_codebook *cb, float r, int64_t group_first, int64_t group_count,
                                    float *qerror_out);
int  somhip_batchmap_missing_end(somhip_codebook *cb);
int  somhip_batchmap_missing_state(somhip_codebook *cb, void **dev_state, int64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* SOMHIP_BATCHMAP_MISSING_H */
