/* somhip.h -- C ABI of the MI355X (gfx950) SOM/LVQ training engine.
 *
 * This is the drop-in boundary for the hot path of SOM_PAK/LVQ_PAK 3.2
 * (hynde/som_lvq_pak): best-matching-unit search + codebook update inside the
 * vsom / lvqtrain epoch loops, and the read-only winner scans of qerror /
 * accuracy / vcal.  Plain C: opaque handles, plain pointers and sizes, int status
 * (0 = ok, nonzero = error; text via somhip_last_error()).  Nothing here aborts and no
 * C++ exception crosses this boundary; a failing call leaves a message and returns
 * nonzero, the way the reference's training functions return NULL and print to stderr
 * (som_rout.c:576-596).
 *
 * One host thread per engine (the reference is single-threaded and not re-entrant,
 * SURVEY.md 8b); one engine per process per GPU.
 *
 * Each entry point cites the reference interface it replaces (file:line in
 * hynde/som_lvq_pak).  INTEGRATION.md shows the reference-side binding.
 */
#ifndef SOMHIP_H
#define SOMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SOMHIP_VERSION 1

/* ids equal to the reference's (lvq_pak.h:209-224) */
enum { SOMHIP_TOPOL_LVQ = 2, SOMHIP_TOPOL_HEXA = 3, SOMHIP_TOPOL_RECT = 4 };
enum { SOMHIP_NEIGH_BUBBLE = 1, SOMHIP_NEIGH_GAUSSIAN = 2 };
enum { SOMHIP_ALPHA_LINEAR = 1, SOMHIP_ALPHA_INVERSE_T = 2 };
enum { SOMHIP_LVQ1 = 1, SOMHIP_OLVQ1 = 2, SOMHIP_LVQ2 = 3, SOMHIP_LVQ3 = 4 };

/* winner tie rules: FIRST = find_winner_euc (lowest index among equal distances,
 * lvq_pak.c:79); KNN = find_winner_knn with knn >= 2 (later row first, lvq_pak.c:197) */
enum { SOMHIP_TIE_FIRST = 0, SOMHIP_TIE_KNN = 1 };

typedef struct somhip_engine somhip_engine;
typedef struct somhip_codebook somhip_codebook;   /* replaces the `codes` entries list, lvq_pak.h:89-113 */
typedef struct somhip_dataset somhip_dataset;     /* replaces the `data` entries list (one -buffer worth) */

const char *somhip_last_error(void);
int somhip_version(void);

/* GPUs visible to this process (a multi-GPU host: one process per GPU, rank r on device r % count) */
int  somhip_device_count(int *count);

/* ---- engine ---- */
int  somhip_engine_create(int device, somhip_engine **out);
/* Destroying an engine releases the device memory of every codebook / data set created on it; those handles
 * stay valid for their own destroy call (any order of the destroy calls is fine), every other call on them
 * fails with "the engine of this handle was destroyed". */
void somhip_engine_destroy(somhip_engine *e);
/* the HIP stream all work of this engine is enqueued on (a hipStream_t) */
void *somhip_engine_stream(somhip_engine *e);
int  somhip_engine_sync(somhip_engine *e);

/* Winner-search implementation for runs of samples (mini-batch training, find_winners k=1):
 *   SOMHIP_SCAN_DIRECT  direct-form fp32 scan on the vector ALU (the reference's arithmetic)
 *   SOMHIP_SCAN_MFMA    fp32-MFMA distance GEMM as a pre-filter with a rigorous error bound +
 *                       exact re-rank of the surviving rows by the direct-form arithmetic
 *   SOMHIP_SCAN_MFMA_BF16  the same with the GEMM on the bf16 matrix pipe (operands split
 *                       hi + lo, three MFMAs per K-step; wider bound, same exact re-rank)
 * All return bit-identical winners; the MFMA forms apply where there are no masks (default:
 * SOMHIP_SCAN_MFMA_BF16). */
enum { SOMHIP_SCAN_DIRECT = 0, SOMHIP_SCAN_MFMA = 1, SOMHIP_SCAN_MFMA_BF16 = 2 };
int  somhip_engine_set_scan_mode(somhip_engine *e, int mode);
/* How a mini-batch (batch > 1) applies its neighbourhood updates:
 *   SOMHIP_UPDATE_EXACT  adapt_vector's arithmetic, hit after hit (lvq_pak.c:348-349: sub, mul, add, each rounded):
 *                        bit-identical to orc_som_training(batch) in oracle/ -- the default
 *   SOMHIP_UPDATE_GEMM   the same affine map of every unit, c' = P c + sum_j w_j x_j, evaluated as a matrix product
 *                        on the fp32 matrix pipe (kernels/som_update_gemm.hpp); same result up to fp32 rounding of a
 *                        sum instead of a chain, hits whose weight has decayed below 2^-24 skipped; no masked
 *                        components, dim a multiple of 128; gaussian neighbourhoods (maps up to 1024 x 1024): every
 *                        unit's rate per sample as a dense weight matrix, the rates through the fp32 exp
 *                        (otherwise the exact kernels run)
 * batch == 1 (the reference's online algorithm) is not affected.  Environment: SOMHIP_UPDATE_MODE=gemm|exact. */
enum { SOMHIP_UPDATE_EXACT = 0, SOMHIP_UPDATE_GEMM = 1 };
int  somhip_engine_set_update_mode(somhip_engine *e, int mode);
/* cumulative re-rank statistics of the MFMA path since engine creation:
 * out[0] = row groups re-ranked, out[1] = rows re-ranked, out[2] = max groups for one sample,
 * out[3] = samples searched (fewer than the samples trained where somhip_som_train searched only the end of a run, see
 * there), out[4] = (row, iteration) updates applied by mini-batch runs,
 * out[5] = (row group, iteration) pairs with at least one update, out[6] = list entries ((row group, iteration)
 * pairs) the GEMM-form update walked (it stops where the weights have decayed away), out[7] = (row group, sample) pairs
 * that survived level 1 of the two-level pre-filter and went through the three-product level 2 */
int  somhip_scan_stats(somhip_engine *e, uint64_t out[8]);

/* diagnostics (tests): run only the pre-filter of the current scan mode on data rows
 * [first, first+count) and return its raw outputs: wmin[ngroups][*bpad] (group minima of
 * s~ = ||c||^2 - 2<c,x>) and tau[count].  wmin must hold ngroups * (count rounded up to 32). */
int  somhip_debug_prefilter(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                            float *wmin, float *tau, int64_t *bpad);

/* diagnostics (tests): run only the preparation and level 1 of the two-level pre-filter (bf16 scan mode) on data rows
 * [first, first+count), by the persistent ring kernel (ring = 1) or by the wide-tile kernel followed by the pass over
 * the group minima (ring = 0), and return wmin[ngroups][*bpad] (level 1's group minima of s~ = ||c||^2 - 2<c_hi,x_hi>)
 * and gmin1[*bpad] (per sample the smallest of them, as an order-preserving uint32).  *bpad = count rounded up to 32.
 * Refuses shapes that one of the two kernels does not take: rows that are not whole 64-dim steps, fewer than 225
 * samples, more than 65535. */
int  somhip_debug_level1(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int ring,
                         float *wmin, uint32_t *gmin1, int64_t *bpad);

/* diagnostics (tests): run only the preparation of a nearest-row search (bf16 scan mode, a pre-filter route) on data rows
 * [first, first+count) and return what it leaves on the device; every output but info may be null.  With d8 = the
 * 8-dim k-blocks of a row (dims rounded up to 8), ngroups = rows rounded up to 64 over 64, nsb = count rounded up to 32
 * over 32, bf16 values as uint16:
 *   chi, clo [ngroups][d8][64][8]   hi and lo pieces of the codebook's rows (row r of group g at [g][kb][r])
 *   cn [ngroups * 64]               squared row norms, 3.0e38 for padding rows
 *   rowmajor [ngroups * 64][d]      the row-major copy of the rows, where the search makes one (info[0])
 *   xhi, xlo [nsb][d8][32][8]       hi and lo pieces of the samples; xlo only where a kernel reads it (info[1])
 *   xrow [nsb * 32][d8][2][8]       the same pieces sample by sample, hi then lo (two-level route: info[2])
 *   tau [count], tau1 [count]       the windows of the re-rank and of level 1 (tau1: two-level route)
 * info[0] = rowmajor was written, info[1] = xlo was written, info[2] = the route has two levels, info[3] = d8. */
int  somhip_debug_prepared(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                           uint16_t *chi, uint16_t *clo, float *cn, float *rowmajor, uint16_t *xhi, uint16_t *xlo,
                           uint16_t *xrow, float *tau, float *tau1, int32_t info[4]);

/* diagnostics (tests): the codebook's cache of prepared copies as it lies on the device now, left by whatever search or
 * writer ran last, and the flags that say whether a search may trust it.  Nothing is launched and no flag changes; the
 * engine's stream is synchronised.  flags[0] = the tiles and norms describe the rows as they are (prep_valid), flags[1] =
 * so does the row-major copy (rowmajor_valid), flags[2] = a batch-map accumulation is open (bm_open), flags[3] = a
 * somhip_batchmap_finish has written rows from it (bm_moved).  chi, clo, cn, rowmajor: as somhip_debug_prepared sizes
 * them; each may be null, and one the codebook never allocated is left unwritten -- whatever the flags say. */
int  somhip_debug_prepared_state(somhip_codebook *cb, int32_t flags[4], uint16_t *chi, uint16_t *clo, float *cn,
                                 float *rowmajor);

/* diagnostics (tests): the nearest-row search of data rows [first, first+count) on a pre-filter route, with the pairs of
 * the exact re-rank selected from level 2's lists (from_lists = 1, two-level route only: what the search itself does
 * there) or from the whole matrix of group minima (from_lists = 0).  Returns, with *bpad = count rounded up to 32 and
 * ncols = *bpad / 32: wmin, wmask [ngroups][*bpad] (the pre-filter's group minima and row masks as the selection found
 * them), gmin [*bpad] (per-sample minimum, order-preserving uint32), tau [count], colcount [4][ncols] (per 32-sample
 * column: pairs, row groups, rows, largest group count of one sample), *overflow (above ncols * 16384 when a column's
 * 16384-pair segment was full and the whole run went through the group-granular re-rank), pairs [*npairs][2] ((sample,
 * row) of every column's segment, one column after another, at most 16384 of a column; an error if more than pairs_cap)
 * and keys [count] (the search's result). */
int  somhip_debug_rerank_pairs(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int from_lists,
                               float *wmin, uint64_t *wmask, uint32_t *gmin, float *tau, uint32_t *colcount,
                               uint32_t *overflow, uint32_t *pairs, int64_t pairs_cap, int64_t *npairs,
                               uint64_t *keys, int64_t *bpad);

/* diagnostics (tests): the route somhip_batch_winner_keys / somhip_batch_topk_keys / somhip_find_winners would take
 * for `count` samples and `want` (1, the top-k width 2/4/8, or a knn of 9 .. SOMHIP_KNN_MAX); host arithmetic only, no
 * GPU work.  (somhip_find_winners searches its run in pieces of at most 4096 samples: ask with the length of a piece.)
 * want 9 .. SOMHIP_KNN_MAX: out[0] = 4 (the wide k-NN route), out[1] = samples per chunk, out[2] as below, the rest 0.
 * out[0] = route (0 masked scan, 1 direct scan, 2 one-level pre-filter, 3 two-level pre-filter), out[1] = kth (level 1's
 * window above the smallest group minimum: 1, or above the 8th smallest), out[2] = split-bf16 GEMMs (else fp32 MFMA),
 * out[3] = level 1 by the persistent ring kernel, out[4] = top-k re-rank filed by row group (else by pair), out[5] =
 * level 2 reads its samples from global memory (else LDS), out[6] = the two-level nearest-row search takes its
 * per-sample minimum from level 2, out[7] = 0 */
int  somhip_debug_scan_plan(somhip_codebook *cb, somhip_dataset *ds, int64_t count, int want, int32_t out[8]);
/* diagnostics (tests): the plan somhip_som_batch_update (and somhip_som_train, per batch) would follow for the mini-batch
 * update of iterations [batch_start_iter, +count) on data rows from data_first: the same arguments but the keys, the
 * same checks; the step scalars are made on the host, nothing is launched.
 * out[0] = apply kernel (0 k_som_update_gemm, 1 k_som_update_gauss_h, 2 k_som_update_gauss_s, 3 k_som_update_bubble_s,
 * 4 k_som_update_run), out[1] = chunks per wave of bubble_s / run (else 0), out[2] = bubble_s with byte offsets,
 * out[3] = gemm's 32-dim tiles per wave (else 0), out[4] = k_decode_winners runs, out[5] / out[6] = k_som_members'
 * threads per workgroup and samples per thread and trip, out[7] = what a member entry carries (0 the sample's index in
 * the run, 1 its row offset in float4 units, 2 in bytes), out[8] = entries carry packed winner coordinates (gaussian
 * gemm), out[9] = only the tail of each list is made, out[10] = its length (0: whole lists), out[11] = the run's largest
 * reach (-1: not used), out[12] = k_order_groups runs, out[13] / out[14] = the apply kernel's grid and workgroup size,
 * out[15] = 0 */
struct somhip_som_params;                          /* (below, with somhip_som_train) */
int  somhip_debug_update_plan(somhip_codebook *cb, somhip_dataset *ds, const struct somhip_som_params *p,
                              int64_t batch_start_iter, int64_t count, int64_t data_first, int32_t out[16]);

/* diagnostics (tests): the device addresses a cached graph of online SOM iterations is keyed by: out[0] = the
 * codebook's tiles, out[1] = the data rows, out[2] = the data mask (0: none) */
int  somhip_debug_device_ptrs(somhip_codebook *cb, somhip_dataset *ds, uint64_t out[3]);

/* ---- codebook mirror -------------------------------------------------------
 * rows: host, row-major [n_rows][dim] fp32, row k = list position k of the
 * reference's codebook (datafile.c:781,836) = map unit (k % xdim, k / xdim)
 * (som_rout.c:641-642).  labels: first label of each row (labels.h:44) or NULL.
 * For a row-sharded codebook (multi-GPU) this process holds global rows
 * [row_offset, row_offset + n_rows) of n_global; single GPU: row_offset 0,
 * n_global == n_rows. */
int  somhip_codebook_create(somhip_engine *e, const float *rows, const int32_t *labels,
                            int64_t n_rows, int dim, int topol, int neigh, int xdim, int ydim,
                            int64_t row_offset, int64_t n_global, somhip_codebook **out);
/* Interleaved shards of a map (multi-GPU SOM training): the map is cut into 8x8-unit patches numbered
 * row-major and shard s of S holds patches s, s+S, s+2S, ...  A neighbourhood (som_rout.c:472-549)
 * of any radius around any winner then covers about 1/S of its units on every shard, so the update
 * work of a batch is the same on all ranks; contiguous blocks of rows load the ranks that hold the
 * middle of the map up to 1.4x the mean.  Map sides must be multiples of 8.
 * somhip_shard_units: the global unit index (k of the comment above) of every row of the shard, in the
 * order in which create_interleaved / download / upload exchange its rows (units == NULL: count only).
 * Keys, traces and winners carry global unit indices as with contiguous shards. */
int  somhip_shard_units(int xdim, int ydim, int shard_index, int shard_count, int64_t *units, int64_t *n_units);
int  somhip_codebook_create_interleaved(somhip_engine *e, const float *rows, int64_t n_rows, int dim,
                                        int topol, int neigh, int xdim, int ydim, int shard_index,
                                        int shard_count, somhip_codebook **out);
/* device -> host gather of the rows (what save_entries / save_snapshot need,
 * datafile.c:353, lvq_pak.c:665) */
int  somhip_codebook_download(somhip_codebook *cb, float *rows);
int  somhip_codebook_upload(somhip_codebook *cb, const float *rows);
void somhip_codebook_destroy(somhip_codebook *cb);

/* ---- data mirror -----------------------------------------------------------
 * rows row-major [n_rows][dim]; optional per-row arrays (NULL = absent):
 *   mask    [n_rows][dim] nonzero = component ignored (data_entry.mask, lvq_pak.h:84)
 *   labels  first label per row                      (labels.h:44)
 *   weight  data_entry.weight                        (lvq_pak.h:81)
 *   fixed_xy [n_rows][2], -1 = none                  (struct fixpoint, lvq_pak.h:65) */
int  somhip_dataset_create(somhip_engine *e, const float *rows, int64_t n_rows, int dim,
                           const uint8_t *mask, const int32_t *labels, const int16_t *weight,
                           const int16_t *fixed_xy, somhip_dataset **out);
/* same, but `dev_rows` already lives in this GPU's memory (row-major fp32) and is
 * used in place, not copied (bench / streaming ingest) */
int  somhip_dataset_wrap_device(somhip_engine *e, const float *dev_rows, int64_t n_rows, int dim,
                                somhip_dataset **out);
/* a data set generated in place: rows [first_row, first_row + n_rows) of the seeded Gaussian-mixture stream
 * (k_centres centres 4z, row = centre[k(row)] + z, z = sum of twelve 16-bit uniforms - 6: counter-based
 * and exact, so it equals the host form bit for bit -- `-din gen:k=..,dim=..,n=..,seed=..` in the C tools,
 * pak_gen_row in som_lvq_pak_amd/host/pak_io.c).  centres (host, may be NULL) receives each row's mixture id,
 * which also becomes the data set's labels.  No host copy, no PCIe: what the C4/C5-sized runs need. */
int  somhip_dataset_generate(somhip_engine *e, uint64_t seed, int k_centres, int dim, int64_t first_row,
                             int64_t n_rows, int32_t *centres, somhip_dataset **out);
/* rows [first, first + count) of the mirror back to the host (generated data sets: picking initial codes) */
int  somhip_dataset_download_rows(somhip_dataset *ds, int64_t first, int64_t count, float *rows);
void somhip_dataset_destroy(somhip_dataset *ds);

/* ---- winner scans: WINNER_FUNCTION over a run of samples (lvq_pak.h:146) -----
 * find_winner_euc (lvq_pak.c:41) when tie == SOMHIP_TIE_FIRST and knn == 1,
 * find_winner_knn (lvq_pak.c:152) when tie == SOMHIP_TIE_KNN (1 <= knn <= SOMHIP_KNN_MAX).
 * knn <= 8 takes the top-k scans (direct, or behind the MFMA pre-filter on big codebooks); 9 <= knn <= SOMHIP_KNN_MAX
 * takes the wide route in every scan mode: exact distances of a chunk of samples to every row, then a select of the
 * knn smallest per sample -- no pre-filter, so its cost is that of the direct scan plus the select.
 * Samples are data rows [first, first+count).  Outputs are host arrays
 * [count][knn]: index = global row (or -1: nothing beat FLT_MAX), diff = SQUARED
 * distance exactly as the reference's fp32 left-to-right sum gives it; ret[i] = the
 * function's return value (knn, or 0 = every component masked). ret may be NULL.
 * Masked data sets (somhip_dataset_create with a mask) work for every knn: only the sample's
 * mask counts (lvq_pak.c:179-186), a code row's own masked components take part with their
 * stored value; a sample with every component masked gets ret 0 and index -2 in all knn slots.
 * Masked runs always take the exact direct-form scan (no MFMA pre-filter).
 * A row shard answers with its own knn nearest rows under global unit indices; a host merges the shards' lists by
 * (diff, later row first). */
#define SOMHIP_KNN_MAX 256
int  somhip_knn_max(void);   /* SOMHIP_KNN_MAX of the library in use */
int  somhip_find_winners(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                         int knn, int tie, int32_t *index, float *diff, int32_t *ret);
/* HIP-event totals of the wide route's two stages since somhip_timing_reset, while somhip_timing_enable is on (they are
 * not in the table of somhip_kernel_count): [0] the distance stage, [1] the select stage; one launch of each per chunk */
int  somhip_knn_timing(somhip_engine *e, int64_t launches[2], double total_ms[2]);
/* The class vote over find_winner_knn's neighbours (knn == 1: find_winner_euc's), formed on the device behind the keys of
 * the search somhip_find_winners would run (same routes, chunks, row wrap and masked data): what knntest.c:101-108,
 * setlabel.c:73-80, correct_by_knn (lvq_rout.c:38-78) and elimin.c:87-101 take from the neighbours.  Host arrays [count]:
 *   found  neighbours found: min(knn, rows) unless every component of the sample is masked (0)
 *   label  the head of the reference's hit list after add_hit (labels.c:370-410) of the found neighbours' labels, nearest
 *          first: the label whose count first reaches the largest count; -1 when found is 0
 *   freq   its count (0 when found is 0)
 *   own    neighbours whose label equals the sample's own label; -1 if the data set was created without labels
 * freq, own and found may be NULL.  The codebook needs labels and must be a whole one: a row shard does not hold the
 * other shards' labels. */
int  somhip_knn_vote(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int knn,
                     int32_t *label, int32_t *freq, int32_t *own, int32_t *found);
/* HIP-event total of the vote kernel since somhip_timing_reset, while somhip_timing_enable is on (like the wide stages,
 * not in the table of somhip_kernel_count); one launch per chunk */
int  somhip_knn_vote_timing(somhip_engine *e, int64_t *launches, double *total_ms);
/* Map quality (K1q): the topographic error and per-unit statistics of a map over data rows (first + s) % n_rows,
 * s = 0 .. count-1, formed on the device behind the top-2 search under SOMHIP_TIE_FIRST (same routes, chunks, row wrap and
 * masked data as somhip_batch_topk_keys).  A sample is searched unless every component of it is masked (find_qerror skips
 * those, som_rout.c:712).  b1, d1: find_winner_euc's winner and its squared distance; b2: the winner among the other
 * rows, lowest index on equal distances (not find_winner_knn's order); b1 and b2 are adjacent when the squared lattice
 * distance of hexa_dist / rect_dist (som_rout.c:434) is <= 1: the units a bubble of radius 1 around b1 teaches.
 *   out->searched      searched samples
 *   out->topo_defined  ... that have a b2 (none on a map of one unit)
 *   out->topo_errors   ... whose b1 and b2 are not adjacent
 *   out->qerror        find_qerror's float chain (som_rout.c:715) continued from qerror_in over the searched samples in
 *                      data order: the float the qerror tool sums, bit for bit
 *   hits[u]           += searched samples with b1 == u
 *   qsum[u]           += sqrt((double)d1) of those samples, one fp64 addition each, in data order
 * hits and qsum (host arrays of n_rows of the codebook, either may be NULL) are read, continued and written back, so a run
 * cut into several calls at any point -- passing the arrays and the last out->qerror on -- gives the bits of one call.
 * The codebook must be a whole map (xdim * ydim rows, hexa or rect); count >= 2^32 is refused; count <= 0 does nothing. */
typedef struct { int64_t searched, topo_defined, topo_errors; float qerror; } somhip_quality_totals;
int  somhip_map_quality(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                        uint32_t *hits /*[n_rows] in/out or NULL*/, double *qsum /*[n_rows] in/out or NULL*/,
                        float qerror_in, somhip_quality_totals *out);
/* HIP-event totals of its two kernels since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count): [0] the pair pass, [1] the unit pass; one launch of each per chunk */
int  somhip_map_quality_timing(somhip_engine *e, int64_t launches[2], double total_ms[2]);
/* Map connectivity (K1c; no reference function): CADJ(i, j), the number of samples whose best unit is i and second-best
 * unit j -- the cumulative adjacency matrix of Tasdemir and Merenyi (CONN = CADJ + its transpose), and on a codebook
 * without a lattice the edges competitive Hebbian learning draws (Martinetz and Schulten).  Searched, b1, b2 are K1q's
 * above; a sample is defined when it is searched and has both.  Units are unit indices u = y * xdim + x.
 * A somhip_conn is a pair table on the device, owned by the caller: the pairs with a non-zero count, ascending by (i, j),
 * each with a 64-bit count.  It is a handle like a codebook: destroying the engine first releases its device memory, after
 * which every call on it but somhip_conn_destroy fails with a message.
 *   somhip_conn_clear   empties the table (it may then take the pairs of a codebook of another size)
 *   somhip_conn_size    *pairs = entries, *samples = the sum of their counts (either may be NULL)
 *   somhip_conn_read    entries [first, first + n) in table order into b1, b2, count (each may be NULL); refused outside
 *                       [0, pairs]
 * somhip_map_connectivity adds the pairs of data rows (first + s) % n_rows, s = 0 .. count-1, to the table.  Every result
 * is an integer: a run cut into any number of calls, over one data set or several, leaves the same table.
 *   out == NULL   that alone; any codebook that is not a shard, with a lattice or without; hits and qsum must be NULL
 *   out != NULL   somhip_map_quality beside it, from the same search: the same refusals and the same bits in hits, qsum
 *                 and out
 * Refused before anything is launched, the table untouched: null handles, handles of different engines or of a destroyed
 * one, different dimensions, a row shard, first < 0, count >= 2^32, a table that holds pairs of a codebook with another
 * number of units.  count <= 0 does nothing.  The keys of SOMHIP_CONN_SLAB samples are sorted at a time: the device memory
 * of a call is that slab's and the table's, whatever count is.
 * somhip_conn_timing: HIP-event totals since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count): [0] the key pass (one launch per chunk), [1] the sort, [2] the run pass, [3] the merge (per slab:
 * one, three and three timed scopes). */
typedef struct somhip_conn somhip_conn;
#define SOMHIP_CONN_SLAB 1048576
int  somhip_conn_create(somhip_engine *e, somhip_conn **out);
void somhip_conn_destroy(somhip_conn *c);
int  somhip_conn_clear(somhip_conn *c);
int  somhip_conn_size(somhip_conn *c, int64_t *pairs, uint64_t *samples);
int  somhip_conn_read(somhip_conn *c, int64_t first, int64_t n, uint32_t *b1, uint32_t *b2, uint64_t *count);
int  somhip_map_connectivity(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, somhip_conn *c,
                             uint32_t *hits /*[n_rows] in/out or NULL*/, double *qsum /*[n_rows] in/out or NULL*/,
                             float qerror_in, somhip_quality_totals *out /* or NULL */);
int  somhip_conn_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]);

/* ---- som_training (som_rout.c:556-671) --------------------------------------
 * Runs iterations [start_iter, start_iter+count) of a schedule of `length`
 * iterations; iteration le uses data row (data_first + (le - start_iter)) % n_rows.
 * batch == 1: the reference's strictly online algorithm, bit-exact.
 * batch  > 1: mini-batch schedule -- the winners of each run of `batch` iterations
 *             are found against the codebook as it stood before the run, then the
 *             neighbourhood updates are applied in iteration order (exact oracle:
 *             orc_som_training(batch) in oracle/).
 * batch == SOMHIP_BATCH_AUTO: the mini-batch schedule with the engine's own batch sizes (somhip_som_auto_batch):
 *             long batches while the end state still forgets them, short ones after -- or batch 1 where that rule
 *             has not been measured against the online engine (small maps, short runs).  Measured at configs[3]'s
 *             real length on three seed pairs (profiles/r03_conformity_*.jsonl).
 * trace_index/trace_diff (host, [count], may be NULL): winner of every iteration;
 * -2 = skipped (sample fully masked), -3 = fixed-point sample (no search).
 * Lazy search: with no trace wanted, update mode gemm and a bubble neighbourhood that covers a good part of the map, a
 *             run's winners are searched only for its last M samples (whole trips of k_som_members, at most half the
 *             run): the GEMM update reads each row group's list from its end and stops where the weights have decayed
 *             below 2^-24, so the samples in front of every group's tail change nothing.  k_som_members counts the
 *             groups whose tail did not fill within M; the host reads that word (the loop's only host wait) and, if it
 *             is not zero, searches the rest of the run and makes the lists again.  The codebook, and the update
 *             statistics of somhip_scan_stats, are those of the full search, bit for bit; `samples searched` is
 *             smaller.  With a trace, and through somhip_batch_winner_keys + somhip_som_batch_update, every sample is
 *             searched. */
#define SOMHIP_BATCH_AUTO (-1)
typedef struct somhip_som_params {
  int64_t length;        /* teach_params.length  (lvq_pak.h:198) */
  float   alpha;         /* teach_params.alpha   (lvq_pak.h:197) */
  float   radius;        /* teach_params.radius  (lvq_pak.h:196) */
  int32_t alpha_type;    /* teach_params.alpha_type (lvq_pak.h:189) */
  int32_t use_fixed;     /* use_fixed(-1)   (lvq_pak.c:508) */
  int32_t use_weights;   /* use_weights(-1) (lvq_pak.c:519) */
  int64_t batch;
  int64_t start_iter, count, data_first;
} somhip_som_params;
int  somhip_som_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_som_params *p,
                      int32_t *trace_index, float *trace_diff);
/* The batch of the SOMHIP_BATCH_AUTO schedule that holds iteration `iter`: [*batch_start, *batch_start + *batch_len).
 * p: length, alpha, alpha_type, radius of the run (teach_params, lvq_pak.h:186-204); n_units = xdim * ydim of the WHOLE map
 * (also on a shard), topol / neigh as in the codebook.  The schedule is a rule in (n_units, radius(t), alpha(t)) --
 * csrc/host_som.inc, som_auto_plan: 32768 iterations per batch while what a batch leaves in the map is forgotten again by
 * the end of the run (the sum F(t) of alpha(t') x the share of the map one sample teaches over the rest of the run is
 * >= 64), 8192 after (configs[3]: 32768 up to iteration 8 486 912 of 10 M, then 8192; where the line lies was measured
 * on three seed pairs).  Where the rule is not vouched for by a measurement
 * against the online engine -- maps below 16384 units, runs whose long phase holds fewer than 64 long batches -- every
 * batch is ONE iteration: `auto` is then the reference's own online schedule (bit-exact).
 * A host that drives somhip_batch_winner_keys / somhip_som_batch_update itself (one process per GPU) asks this
 * function for its batch boundaries, so that every rank cuts the run the same way.  Plain host arithmetic: no GPU needed. */
int  somhip_som_auto_batch(const somhip_som_params *p, int64_t n_units, int topol, int neigh, int64_t iter,
                           int64_t *batch_start, int64_t *batch_len);

/* ---- the batch map (K8; no reference function) -----------------------------------
 * Kohonen's batch map: every epoch finds the winners of the whole data set against the frozen codebook and replaces
 * every model vector by the neighbourhood-weighted mean of the data.  No learning rate, no dependence on the order of
 * the data.  (batch > 1 of somhip_som_train is something else: mini-batches of the ONLINE rule.)
 * One call runs epochs t = start_epoch .. start_epoch + count - 1 of a run of T = epochs epochs over data rows
 * (first + s) % n_rows, s = 0 .. n-1.  Per epoch:
 *   1. r_t = 1.0f + (radius - 1.0f) * (float)(T - t) / (float)T, in float (som_rout.c:615 with le -> t, length -> T)
 *   2. c(s) = find_winner_euc of sample s against the codebook as the epoch found it: the lowest index among equal
 *      distances (SOMHIP_TIE_FIRST)
 *   3. hits[j] = the samples with c(s) = j (uint32); S[j][k] = the sum of (double)x_s[k] over them, ONE chain of fp64
 *      additions from +0.0 in data order: the same bits on every run, no floating-point atomics
 *   4. h(i, j) from the units' lattice positions with hexa_dist / rect_dist.  bubble: 1 where the online kernels'
 *      membership test holds (bit-equal with dist <= r_t, som_rout.c:496), else 0; gaussian:
 *      exp((double)(-dd * dd / (2.0 * r_t * r_t))), dd the float lattice distance (som_rout.c:808)
 *   5. N[i][k] = sum_j h(i,j) S[j][k], D[i] = sum_j h(i,j) hits[j] in fp64 (v_mfma_f64_16x16x4_f64; the order over j is
 *      the storage order of the rows, a function of the shape alone); m_i[k] = (float)(N[i][k] / D[i]) where D[i] > 0, a
 *      row with D[i] == 0 keeps its bits
 * qerror_out (host, [count], or NULL): per epoch the quantization error of the codebook the epoch started from, the
 * float chain of find_qerror over the winners' distances in data order (as somhip_map_quality forms it).  NULL: no
 * per-sample copy leaves the device.
 * Refused, with a message that names the entry point, before anything is launched: data with x components, sharded
 * codebooks, codebooks without a lattice, n >= 2^32, n <= 0, first < 0, epochs < 1, radius < 1, epochs outside
 * [0, epochs).  Fixed points and weights are not taken. */
typedef struct somhip_batchmap_params {
  int64_t epochs;        /* T */
  float   radius;        /* the radius the run starts from */
  int64_t start_epoch, count;
  int64_t first, n;      /* the data rows of every epoch */
} somhip_batchmap_params;
int  somhip_som_batchmap(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p,
                         float *qerror_out /*[count] or NULL*/);
/* The two stages somhip_som_batchmap is made of, each on its own.  _sums: steps 2-3 -- hits[n_rows of the codebook],
 * sums[n_rows][dim] to the host.  _combine: steps 4-5 at radius r (>= 0) on host-supplied hits and sums; it writes the
 * codebook. */
int  somhip_debug_batchmap_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, uint32_t *hits,
                                double *sums);
int  somhip_debug_batchmap_combine(somhip_codebook *cb, float r, const uint32_t *hits, const double *sums);
/* HIP-event totals of its stages since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count): [0] group (the winners pass per chunk, the scan of the counts, the sort by winner), [1] the
 * sums, [2] the combine (with the gaussian table) */
int  somhip_batchmap_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]);
/* The same epoch over data that comes in pieces.  S[j][k] is a chain of additions, and a chain can be continued: where a
 * piece's sums start from the S the pieces before it left instead of from +0.0, any cut of the data -- into buffers, into
 * calls, into the row blocks of G ranks -- leaves the bits of one call.  Only the sums are serial across the pieces; the
 * winner search runs per piece.
 *   _begin       allocates, or re-zeroes, a state the codebook owns (not engine scratch: other engine calls between the
 *                pieces leave it alone): [S | hits] as n_rows x (dim + 1) doubles, all +0.0, and a tail of 16 bytes
 *                {float q; uint32 unused; uint64 samples}
 *   _accumulate  steps 2-3 over rows (first + s) % n_rows, s < n, of ds, a data set of the codebook's engine and dimension
 *                (the pieces may come from different data sets; each wraps inside its own): the chains go on from S, the
 *                counts grow (exact in fp64); want_qerror: find_qerror's float chain goes on over the piece as well
 *   _finish      steps 4-5 at radius r (>= 0) for the destination row groups (64 rows of the codebook's storage order)
 *                [group_first, group_first + group_count) of (n_rows + 63) / 64; rows of other groups keep their bits.  It
 *                reads S, not the rows, so it may be called again for other ranges; qerror_out (or NULL) gets the q chain.
 *                After the first _finish further pieces are refused ("the codebook has moved") until the next _begin.
 *   _end         frees the state (somhip_codebook_destroy does too)
 *   _state       the device address and the size of the one blob that is the whole state -- the engine keeps nothing of
 *                an accumulation on the host between calls.  Copied into another codebook of the same shape, on this or
 *                another engine, whose own state _begin has opened, it continues the accumulation there.
 * begin, accumulate over the pieces in order, finish(r, 0, ngroups, &q) leaves the codebook and q with the bits one epoch
 * of somhip_som_batchmap at radius r leaves, over a data set whose rows are the pieces' rows in that order.
 * Refused by name before anything is launched, codebook and state untouched: what somhip_som_batchmap refuses (masked
 * data, sharded codebooks, codebooks without a lattice, n <= 0, first < 0); _accumulate / _finish / _state without _begin; a
 * piece of another dimension; a piece that would take the total to 2^32 samples; r < 0; a group range outside
 * [0, ngroups].  A call that writes the codebook's rows while a state is open (upload, the trainings,
 * somhip_som_batchmap) closes the state.  The launches count under the three ids of somhip_batchmap_timing. */
int  somhip_batchmap_begin(somhip_codebook *cb);
int  somhip_batchmap_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int want_qerror);
int  somhip_batchmap_finish(somhip_codebook *cb, float r, int64_t group_first, int64_t group_count, float *qerror_out);
int  somhip_batchmap_end(somhip_codebook *cb);
int  somhip_batchmap_state(somhip_codebook *cb, void **dev_state, int64_t *bytes);

/* ---- batch GLVQ (K9; no reference function) ---------------------------------------
 * Sato and Yamada's Generalized LVQ as full-batch gradient steps: E = mean_s f(mu_s), mu = (d+ - d-) / (d+ + d-), d+ the
 * squared distance to the nearest row of the sample's class and d- to the nearest row of any other class.  No dependence
 * on the order of the data beyond the order of its sums; the same bits on every run.
 * One call runs epochs t = start_epoch .. start_epoch + count - 1 of a run of T = epochs epochs over data rows
 * (first + s) % n_rows, s = 0 .. n-1.  Per epoch:
 *   1. alpha_t = alpha * (float)(T - t) / (float)T, in float (LVQ_PAK's linear rate)
 *   2. per sample, against the codebook as the epoch found it: (d+, i+) = the smallest find_winner_euc squared distance
 *      (fp32: sub, mul, add in dimension order, three roundings) over the rows whose label equals the sample's, and that
 *      row; (d-, i-) the same over the rows whose label differs; the lowest row index among equal distances
 *   3. per sample in fp64, every operation one rounding in the order written: dp = (double)d+, dm = (double)d-,
 *      D = dp + dm; identity (sigmoid_beta == 0): mu = (dp - dm) / D, f = mu, fp = 1; sigmoid: f = 1 / (1 + exp(-beta * mu)),
 *      fp = beta * f * (1 - f); xi+ = ((4.0 * fp) * dm) / (D * D), xi- = ((4.0 * fp) * dp) / (D * D); D == 0: mu = 0,
 *      xi+ = xi- = 0.  The sample counts as correct when the key (d+, i+) is smaller than the key (d-, i-)
 *   4. per row j, each sum ONE chain of fp64 additions from +0.0 in data order, no floating-point atomics: over the samples
 *      with i+ = j: Sp[j][k] = sum xi+ * (double)x[k] (multiply, then add), sp[j] = sum xi+, cost[j] = sum f, np[j] their
 *      number (uint32); over the samples with i- = j: Sm[j][k] = sum xi- * (double)x[k], sm[j] = sum xi-, nm[j]
 *   5. with W = (double)w_j[k] and a = (double)alpha_t / (double)n: g = (Sp[j][k] - sp[j] * W) - (Sm[j][k] - sm[j] * W),
 *      w_j[k] = (float)(W + a * g); a row with np[j] == nm[j] == 0 keeps its bits
 * cost_out (host, [count], or NULL): per epoch (the fp64 chain over cost[j] in row order, formed on the host) / n;
 * correct_out (host, [count], or NULL): the number of correct samples.  Both describe the codebook the epoch started from.
 * alpha has the unit of a squared distance (the step is alpha_t times a mean of xi (x - w), and xi is 1 / distance^2).
 * Refused, with a message that names the entry point, before anything is launched and with the codebook untouched: a
 * codebook or data set without labels, x components in the data, a sharded codebook, a dimension mismatch, a data label no
 * codebook row carries, a codebook whose rows all carry one label, n <= 0, n >= 2^32, first < 0, epochs < 1, epochs
 * outside [0, epochs), alpha negative or NaN, sigmoid_beta negative or NaN.  Fixed points and weights are not taken. */
typedef struct somhip_glvq_params {
  int64_t epochs;        /* T */
  int64_t start_epoch, count;
  int64_t first, n;      /* the data rows of every epoch */
  float   alpha;         /* the rate the run starts from */
  float   sigmoid_beta;  /* 0: f is the identity */
} somhip_glvq_params;
int  somhip_glvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_glvq_params *p, double *cost_out /*[count] or NULL*/,
                       int64_t *correct_out /*[count] or NULL*/);
/* The stages somhip_glvq_train is made of, each on its own.
 * _search: step 2 to the host, dplus / dminus [n] and iplus / iminus [n].  route: SOMHIP_GLVQ_DIRECT -- every sample
 * against every row by the class-wise scan; SOMHIP_GLVQ_LIST -- the engine's exact top-8 lists, each role's first entry,
 * and the class-wise scan over the samples whose list lacks a role; SOMHIP_GLVQ_PLAN -- what the training takes for this
 * shape (somhip_debug_glvq_plan).  remainder (or NULL): the samples that went through the class-wise scan.
 * _sums: steps 2-4 to the host: xi_plus, xi_minus, f [n]; sums_plus, sums_minus [n_rows of the codebook][dim + 1], the
 * last column sp / sm; n_plus, n_minus, cost [n_rows]; *correct.
 * _update: step 5 with a = (double)alpha_t / (double)n on host-supplied sums; it writes the codebook. */
#define SOMHIP_GLVQ_PLAN   (-1)
#define SOMHIP_GLVQ_DIRECT 0
#define SOMHIP_GLVQ_LIST   1
int  somhip_debug_glvq_plan(int64_t n_rows, int dim, int64_t n, int32_t *route);
int  somhip_debug_glvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int route, float *dplus,
                              int32_t *iplus, float *dminus, int32_t *iminus, int64_t *remainder);
int  somhip_debug_glvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta,
                            double *xi_plus, double *xi_minus, double *f, double *sums_plus, uint32_t *n_plus,
                            double *sums_minus, uint32_t *n_minus, double *cost, int64_t *correct);
int  somhip_debug_glvq_update(somhip_codebook *cb, float alpha_t, int64_t n, const double *sums_plus, const uint32_t *n_plus,
                              const double *sums_minus, const uint32_t *n_minus);
/* HIP-event totals of its stages since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count): [0] the search (the list route as one span around the top-8 search, the pick and the remainder's
 * scan), [1] the terms and the grouping (scans of the counts, sorts by winner), [2] the sums, [3] the update */
int  somhip_glvq_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]);

/* ---- batch neural gas (K10; no reference function) ---------------------------------
 * Martinetz and Schulten's neural gas in its batch form (Cottrell, Hammer, Hasenfuss, Villmann 2006): the vector
 * quantizer for a codebook with neither a lattice nor labels.  Every sample feeds its first K ranked units with the
 * weight exp(-rank / lambda); every unit becomes the weighted mean of what it was fed.  No learning rate, no dependence on
 * the order of the data beyond the order of its sums; the same bits on every run.
 * One call runs epochs t = start_epoch .. start_epoch + count - 1 of a run of T = epochs epochs over data rows
 * (first + s) % n_rows, s = 0 .. n-1, on a codebook of `units` rows.  Per epoch:
 *   1. in double on the host: lambda_t = lambda0 * pow(lambda_end / lambda0, (double)t / (double)(T - 1)) (T == 1: lambda0);
 *      K_t = ranks if ranks > 0, else min(units, SOMHIP_KNN_MAX, 1 + floor(17.0 * lambda_t)); w[r] = exp(-(double)r /
 *      lambda_t), r < K_t.  17 is the smallest integer with exp(-17) < 2^-24: a rank the rule drops weighs less than half
 *      an ulp of the float a row is stored in, relative to rank 0 -- a constant of the definition, not a knob
 *   2. per sample, against the codebook as the epoch found it: its K_t nearest rows by find_winner_euc's squared distance
 *      (fp32: sub, mul, add in dimension order, three roundings), equal distances in find_winner_knn's order (the later
 *      row first) at every K_t -- K_t == 1 on two rows and more takes the first of the two nearest, so the order of ties
 *      does not change along a run; a one-row codebook has one rank
 *   3. per unit j, over the samples that rank j at some r < K_t, in data order, no floating-point atomics:
 *      S[j][k] = ONE chain of fp64 additions from +0.0 of w[r] * (double)x_s[k] (a multiply, then an add, no FMA),
 *      W[j] = the same chain over w[r] alone, hits[j] = the number of such samples (uint32)
 *   4. m_j[k] = (float)(S[j][k] / W[j]) where W[j] > 0; a unit outside every sample's first K_t ranks, or whose weights all
 *      underflowed to zero, keeps its bits
 * On codebooks of at most SOMHIP_KNN_MAX (256) rows, while 17 lambda_t >= units - 1, this is neural gas without any
 * truncation.  Beyond 256 rows it is neural gas TRUNCATED at the 256 nearest units of every sample: no rank past the
 * 256th is ever fed, whatever lambda is.
 * qerror_out (host, [count], or NULL): per epoch find_qerror's float sum over the rank-0 distances in data order -- the
 * quantization error of the codebook the epoch started from; NULL: no per-sample copy leaves the device.
 * Any whole codebook is taken, with or without a lattice, with or without labels; header and labels are not touched.  It
 * closes an open batch-map state, like the other writers of the rows.
 * Refused, with a message that names the entry point, before anything is launched and with the rows untouched: data with x
 * components, sharded codebooks, a dimension mismatch, n <= 0, n >= 2^32, first < 0, epochs < 1, lambda0 not > 0,
 * lambda_end not in (0, lambda0], ranks outside 0 .. 256, epochs outside [0, epochs). */
typedef struct somhip_ng_params {
  int64_t epochs;        /* T */
  double  lambda0;       /* the neighbourhood range, in ranks, the run starts from */
  double  lambda_end;    /* ... and ends at */
  int64_t ranks;         /* 0: K_t by the rule above; 1 .. 256: K_t of every epoch */
  int64_t start_epoch, count;
  int64_t first, n;      /* the data rows of every epoch */
} somhip_ng_params;
int  somhip_ng_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_ng_params *p, float *qerror_out /*[count] or NULL*/);
/* The stages somhip_ng_train is made of, each on its own.
 * _schedule: step 1 of epoch t for a codebook of `units` rows, on the host (no GPU): *lambda, *K and weights[256], zeros
 * behind K.
 * _ranks: step 2 to the host, units_out / dist_out [n][K] (K 1 .. 256): the r-th nearest unit and its squared distance,
 * -1 / -1.0f where the codebook has no r-th row below FLT_MAX.
 * _sums: steps 2-3 with K ranks and host-supplied weights[K]: hits [units], sums [units][dim], wsum [units] to the host.
 * The data go through in segments of `segment` samples (<= 0: the engine's own rule, at most 2^24 (sample, rank) pairs a
 * segment); the segments after the first continue the chains, so every segment length leaves the same bits.
 * _update: step 4 on host-supplied sums and wsum (hits: as _sums returns them; W decides which rows move); it writes the
 * codebook. */
int  somhip_debug_ng_schedule(const somhip_ng_params *p, int64_t units, int64_t t, double *lambda, int32_t *K, double *weights /*[256]*/);
int  somhip_debug_ng_ranks(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int K, int32_t *units_out,
                           float *dist_out);
int  somhip_debug_ng_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int K, const double *weights,
                          int64_t segment, uint32_t *hits, double *sums, double *wsum);
int  somhip_debug_ng_update(somhip_codebook *cb, const uint32_t *hits, const double *sums, const double *wsum);
/* HIP-event totals of its stages since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count): [0] the entries pass per chunk and the grouping (scan of the counts, sort by unit), [1] the sums,
 * [2] the update.  The search's launches count under their own ids (somhip_timing_get, somhip_knn_timing). */
int  somhip_ng_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]);

/* ---- batch GRLVQ (K11; no reference function) --------------------------------------
 * Hammer and Villmann's relevance GLVQ as full-batch gradient steps: batch GLVQ (above) under the weighted metric
 *   d_lambda(x, w) = sum_k lambda[k] * (x[k] - w[k])^2 ,  lambda[k] >= 0,
 * whose weights, the relevances, are learned by the gradient that moves the rows.  lambda is a host float[dim] the caller
 * owns: read on entry, written on return, never normalised on entry.  So five calls of one epoch that hand lambda on equal
 * one call of five, and lambda all 1.0f with eps = 0 gives somhip_glvq_train's codebook, cost and count bit for bit.
 * One call runs epochs t = start_epoch .. start_epoch + count - 1 of a run of T = epochs epochs over data rows
 * (first + s) % n_rows, s = 0 .. n-1.  Per epoch, everything against the codebook and the lambda the epoch started from:
 *   1. alpha_t = alpha * (float)(T - t) / (float)T and eps_t = eps * (float)(T - t) / (float)T, in float
 *   2. (d+, i+) and (d-, i-) as in somhip_glvq_train step 2, the distance being the weighted fp32 chain in dimension order
 *      from +0.0f: t = c - x, u = lambda[k] * t, p = u * t, acc = acc + p -- four separately rounded operations, no FMA; the
 *      lowest row index among equal distances.  With lambda[k] == 1.0f this is the unweighted chain bit for bit
 *   3. somhip_glvq_train step 3, unchanged: xi+, xi-, f, correct
 *   4. somhip_glvq_train step 4, unchanged: Sp, sp, cost, np; Sm, sm, nm.  Beside them, per row j and component k,
 *      Rp[j][k] = ONE chain of fp64 additions from +0.0 over the samples with i+ = j in data order of
 *      td = (double)x[k] - (double)w_j[k], tt = td * td, pr = xi+ * tt, acc += pr, every operation one rounding;
 *      Rm[j][k] the same over the samples with i- = j, with xi-
 *   5. G[k] = one chain from +0.0 over the rows j = 0 .. rows-1 in unit order of (Rp[j][k] - Rm[j][k]), a subtraction and
 *      then an addition.  No floating-point atomics anywhere
 *   6. with W = (double)w_j[k], a = (double)alpha_t / (double)n and g as in somhip_glvq_train step 5:
 *      w_j[k] = (float)(W + (a * (double)lambda[k]) * g); a row with np[j] == nm[j] == 0 keeps its bits
 *   7. only where eps_t > 0, in IEEE fp64 on the host: e = (double)eps_t / (2.0 * (double)n),
 *      l[k] = (double)lambda[k] - e * G[k], negative values become 0.0, s = the chain of l[k] in order from +0.0; where
 *      s > 0: lambda[k] = (float)(l[k] / s), otherwise lambda keeps its bits.  With eps_t == 0 lambda is neither stepped
 *      nor normalised
 * cost_out, correct_out: as somhip_glvq_train's, under d_lambda; they describe the state the epoch started from.
 * Only the class-wise scan searches here: the pre-filters behind the top-8 lists are unweighted.
 * Refused, with a message that names the entry point, before anything is launched and with the codebook and lambda
 * untouched: everything somhip_glvq_train refuses; a NULL lambda; a lambda[k] that is negative, NaN or infinite; lambda
 * summing to zero; eps negative or NaN. */
typedef struct somhip_grlvq_params {
  int64_t epochs;        /* T */
  int64_t start_epoch, count;
  int64_t first, n;      /* the data rows of every epoch */
  float   alpha;         /* the rate of the rows the run starts from */
  float   sigmoid_beta;  /* 0: f is the identity */
  float   eps;           /* the rate of the relevances the run starts from; 0: lambda stays as given */
} somhip_grlvq_params;
int  somhip_grlvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_grlvq_params *p, float *lambda /*[dim], in and out*/,
                        double *cost_out /*[count] or NULL*/, int64_t *correct_out /*[count] or NULL*/);
/* Step 2 to the host, with lambda given: dplus / dminus [n] and iplus / iminus [n].  What evaluating a trained model needs:
 * a sample is classified correctly when the key (d+, i+) is smaller than the key (d-, i-).  A lambda of zeros is taken
 * (every distance is 0 and the lowest row of either role wins); the other refusals are somhip_grlvq_train's. */
int  somhip_grlvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *lambda, float *dplus,
                         int32_t *iplus, float *dminus, int32_t *iminus);
/* The stages somhip_grlvq_train is made of, each on its own.
 * _sums: steps 2-5 to the host: somhip_debug_glvq_sums' outputs under d_lambda, then rel_plus, rel_minus
 * [n_rows of the codebook][dim] (Rp, Rm) and grad [dim] (G).
 * _update: step 6 with a = (double)alpha_t / (double)n on host-supplied sums, with the lambda given, and then step 7
 * with eps_t and grad: it writes the codebook and lambda. */
int  somhip_debug_grlvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta,
                             const float *lambda, double *xi_plus, double *xi_minus, double *f, double *sums_plus,
                             uint32_t *n_plus, double *sums_minus, uint32_t *n_minus, double *cost, int64_t *correct,
                             double *rel_plus, double *rel_minus, double *grad);
int  somhip_debug_grlvq_update(somhip_codebook *cb, float alpha_t, float eps_t, int64_t n, float *lambda,
                               const double *sums_plus, const uint32_t *n_plus, const double *sums_minus,
                               const uint32_t *n_minus, const double *grad);
/* HIP-event totals of its stages since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count): [0] the weighted class-wise scan, [1] the terms and the grouping (batch GLVQ's stage, counted under
 * its id: somhip_glvq_timing [1] reports the same figures), [2] the sums with the relevance chain, [3] the reduction of
 * the relevance gradient over the rows, [4] the update */
int  somhip_grlvq_timing(somhip_engine *e, int64_t launches[5], double total_ms[5]);

/* ---- batch GMLVQ (K12; no reference function) --------------------------------------
 * Schneider, Biehl and Hammer's matrix relevance GLVQ as full-batch gradient steps: batch GLVQ (above) under the metric
 *   d(x, w) = | Omega (x - w) |^2 ,  Omega of rank (= m) x dim, 1 <= m <= dim,
 * whose matrix is learned by the gradient that moves the rows.  omega is a host float[m][dim], row-major, the caller owns:
 * read on entry, written on return, never normalised on entry.  So five calls of one epoch that hand omega on equal one
 * call of five, and omega the dim x dim identity with eps = 0 gives somhip_glvq_train's codebook, cost and count bit for bit.
 * One call runs epochs t = start_epoch .. start_epoch + count - 1 of a run of T = epochs epochs over data rows
 * (first + s) % n_rows, s = 0 .. n-1.  Per epoch, everything against the codebook and the omega the epoch started from:
 *   1. alpha_t = alpha * (float)(T - t) / (float)T and eps_t = eps * (float)(T - t) / (float)T, in float
 *   2. the projection of every data row and every codebook row z: y[r] = (float)acc_dim with acc_0 = +0.0 and
 *      acc_{k+1} = fma((double)omega[r][k], (double)z[k], acc_k) in fp64, in dimension order (the product of two floats is
 *      exact in fp64, so each step rounds once).  Y = Omega X is [n][m], V = Omega W is [rows][m]
 *   3. (d+, i+) and (d-, i-) exactly as in somhip_glvq_train step 2, on V and Y: the fp32 chain of (c - x)^2 over the m
 *      columns, three separately rounded operations per column, the lowest row index among equal distances
 *   4. somhip_glvq_train step 3, unchanged: xi+, xi-, f, correct
 *   5. somhip_glvq_train step 4, unchanged, on the original rows x: Sp, sp, cost, np; Sm, sm, nm
 *   6. in fp64, with W = (double)w_j[k], a = (double)alpha_t / (double)n and g_j[k] as in somhip_glvq_train step 5:
 *      P[j][r] = ONE chain over k in order from +0.0 of acc + (g_j[k] * (double)omega[r][k]), the product rounded, then
 *      added; Dl[j][k] = one chain over r in order from +0.0 of acc + (P[j][r] * (double)omega[r][k]);
 *      w_j[k] = (float)(W + a * Dl[j][k]); a row with np[j] == nm[j] == 0 keeps its bits
 *   7. the gradient Gm[m][dim].  The run's samples are cut into blocks of 4096 consecutive samples.  Per block and (r, k)
 *      one chain from +0.0 in data order, two steps per sample:  acc = acc + ((xi+ * u+[r]) * t+[k]), then
 *      acc = acc - ((xi- * u-[r]) * t-[k]),  with u+- = (double)y_s[r] - (double)v_{i+-}[r] and
 *      t+- = (double)x_s[k] - (double)w_{i+-}[k], every operation one rounding.  Gm[r][k] = one chain from +0.0 over the
 *      blocks in order.  No floating-point atomics anywhere
 *   8. only where eps_t > 0, in IEEE fp64 on the host: O = (double)omega - ((double)eps_t / (double)n) * Gm, s = the chain
 *      from +0.0 over O * O in row-major order; where s > 0: omega = (float)(O / sqrt(s)), otherwise omega keeps its bits.
 *      With eps_t == 0 omega is neither stepped nor normalised
 * cost_out, correct_out: as somhip_glvq_train's, under the projected distance; they describe the state the epoch started
 * from.  Only the class-wise scan searches here.
 * Refused, with a message that names the entry point, before anything is launched and with the codebook and omega
 * untouched: everything somhip_glvq_train refuses; rank < 1 or rank > dim; a NULL omega; an entry that is NaN or infinite;
 * an omega of zeros; eps negative or NaN. */
typedef struct somhip_gmlvq_params {
  int64_t epochs;        /* T */
  int64_t start_epoch, count;
  int64_t first, n;      /* the data rows of every epoch */
  float   alpha;         /* the rate of the rows the run starts from */
  float   sigmoid_beta;  /* 0: f is the identity */
  float   eps;           /* the rate of omega the run starts from; 0: omega stays as given */
  int32_t rank;          /* m: the rows of omega */
} somhip_gmlvq_params;
int  somhip_gmlvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_gmlvq_params *p, float *omega /*[rank][dim], in and out*/,
                        double *cost_out /*[count] or NULL*/, int64_t *correct_out /*[count] or NULL*/);
/* Steps 2 and 3 to the host, with omega given: dplus / dminus [n] and iplus / iminus [n].  What evaluating a trained model
 * needs: a sample is classified correctly when the key (d+, i+) is smaller than the key (d-, i-).  An omega of zeros is
 * taken (every distance is +0 and the lowest row of either role wins); the other refusals are somhip_gmlvq_train's. */
int  somhip_gmlvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *omega, int32_t rank,
                         float *dplus, int32_t *iplus, float *dminus, int32_t *iminus);
/* Step 2 alone, row-major: with ds, out[n][rank] = the projections of data rows (first + s) % n_rows; with ds NULL,
 * out[rows][rank] = the projections of the codebook's rows in unit order (first and n play no part).  The discriminative
 * picture at rank 2 or 3, and the values the search of step 3 reads. */
int  somhip_gmlvq_project(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *omega, int32_t rank,
                          float *out);
/* The stages somhip_gmlvq_train is made of, each on its own.
 * _sums: steps 2-5 and 7 to the host: somhip_debug_glvq_sums' outputs under the projected distance, then grad [rank][dim] (Gm).
 * _update: step 6 with a = (double)alpha_t / (double)n on host-supplied sums, with the omega given, and then step 8 with
 * eps_t and grad: it writes the codebook and omega. */
int  somhip_debug_gmlvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta,
                             const float *omega, int32_t rank, double *xi_plus, double *xi_minus, double *f, double *sums_plus,
                             uint32_t *n_plus, double *sums_minus, uint32_t *n_minus, double *cost, int64_t *correct,
                             double *grad);
int  somhip_debug_gmlvq_update(somhip_codebook *cb, float alpha_t, float eps_t, int64_t n, float *omega, int32_t rank,
                               const double *sums_plus, const uint32_t *n_plus, const double *sums_minus,
                               const uint32_t *n_minus, const double *grad);
/* HIP-event totals of its stages since somhip_timing_reset, while somhip_timing_enable is on (not in the table of
 * somhip_kernel_count): [0] the projections of the samples and of the rows, [1] the class-wise scan over the projected
 * tiles, [2] the terms and the grouping, [3] the sums (these three are batch GLVQ's stages, counted under its ids:
 * somhip_glvq_timing [0] to [2] report the same figures), [4] the gradient of omega with its reduction over the blocks,
 * [5] the update */
int  somhip_gmlvq_timing(somhip_engine *e, int64_t launches[6], double total_ms[6]);

/* ---- map distortion (K1d; no reference function) ----------------------------------
 * The distortion measure of a map (Lampinen and Oja; SOM Toolbox's som_distortion): its energy at a neighbourhood radius,
 *   E(r) = sum over samples s, sum over units j, of  h_r(c(s), j) * || x_s - m_j ||^2 ,
 * the function one epoch of the batch map minimises for fixed winners.  It is not swept over samples x units x dim: with
 *   1. c(s), hits[c], S[c][k] exactly steps 2-3 of the batch map above (SOMHIP_TIE_FIRST winners, integer counts, one
 *      fp64 chain from +0.0 per (unit, column) in data order)
 *   2. q_s = |x_s|^2 in fp64: lane l of 64 adds (double)x[k] * (double)x[k] (exact) for k = l, l + 64, ... in order from
 *      +0.0, the 64 partials are folded by the xor butterfly 32, 16, 8, 4, 2, 1 -- an order that depends on dim alone;
 *      Q[c] = one chain of fp64 additions of q_s from +0.0 over the unit's samples in data order
 *   3. h(j, c) step 4 of the batch map, at any r >= 0 (bubble at r = 0: E is the plain sum of the squared quantization
 *      errors; gaussian at r = 0 is 0 / 0 on the diagonal by that definition: not a number)
 *   4. [N | D | A] = H x [S | hits | Q] in fp64 (v_mfma_f64_16x16x4_f64; the order over c is the storage order of the rows),
 *      e_j = A_j - 2 sum_k m_jk N_jk + D_j sum_k m_jk^2, formed as A_j + sum_k m_jk (D_j m_jk - 2 N_jk) with the additions
 *      over k and over the blocks of 64 columns in an order fixed by the shape; e_j = 0 where D_j == 0; E = sum_j e_j by a
 *      tree fixed by the number of units.  The same inputs give the same bits on every run; no floating-point atomics.
 *   5. scale = sum_j 2 * (A_j + D_j |m_j|^2) bounds the sum of the absolute values of all terms of E (2 |m.x| <= |m|^2 +
 *      |x|^2).  E resolves about 2^-52 * scale: for data far from the origin scale >> E, and scale / E says how many of E's
 *      digits mean anything.  Centre such data first.
 * A somhip_distortion is a state on the device, the caller's, made for the engine, the number of units and the dimension
 * of the codebook given to _create: [S | hits] as n_rows x (dim + 1) doubles, Q[n_rows], the samples taken.  A handle like
 * a codebook: destroying the engine first releases its device memory, after which every call on it but _destroy fails.
 *   _clear       back to all +0.0 and no samples
 *   _accumulate  steps 1-2 over rows (first + s) % n_rows, s < n, of ds against the codebook's rows as they are: the chains
 *                and counts go on from what the calls before left, so any cut of the data into calls, buffers or data sets
 *                leaves the bits of one call.  The caller keeps the codebook frozen between the pieces.
 *   _evaluate    steps 3-5 at radius r against the codebook's CURRENT rows (the energy of other rows under the accumulated
 *                winners may be asked for): unit_out[n_rows] (or NULL) = e_j by unit, totals.  It writes nothing but its
 *                outputs: the codebook, its prepared copies and an open somhip_batchmap_* state stay as they are.
 *   _read        the state to the host: hits[n_rows], sums[n_rows][dim], sq[n_rows] (each may be NULL)
 * somhip_debug_distortion_evaluate: the evaluate stage on host-supplied hits, sums and sq.
 * Refused by name before anything is launched, state and codebook untouched: null handles, handles of different engines
 * or of a destroyed one, data with x components, sharded codebooks, codebooks without a lattice, a codebook or data set
 * whose shape is not the state's, first < 0, n <= 0, a piece that takes the total to 2^32 samples, r < 0 or NaN.
 * somhip_distortion_timing: HIP-event totals since somhip_timing_reset, while somhip_timing_enable is on (not in the table
 * of somhip_kernel_count): [0] group (the winners pass per chunk, the scan, the sort), [1] the sums and the two Q passes,
 * [2] evaluate (the gaussian table, the kernel, the two fold passes). */
typedef struct somhip_distortion somhip_distortion;
typedef struct somhip_distortion_totals {
  double   energy;       /* E(r) */
  double   scale;        /* E resolves about 2^-52 * scale */
  uint64_t samples;      /* the samples accumulated */
} somhip_distortion_totals;
int  somhip_distortion_create(somhip_codebook *cb, somhip_distortion **out);
void somhip_distortion_destroy(somhip_distortion *st);
int  somhip_distortion_clear(somhip_distortion *st);
int  somhip_distortion_accumulate(somhip_distortion *st, somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n);
int  somhip_distortion_evaluate(somhip_distortion *st, somhip_codebook *cb, float r, double *unit_out /*[n_rows] or NULL*/,
                                somhip_distortion_totals *totals);
int  somhip_distortion_read(somhip_distortion *st, uint32_t *hits, double *sums, double *sq);
int  somhip_debug_distortion_evaluate(somhip_codebook *cb, float r, const uint32_t *hits, const double *sums, const double *sq,
                                      double *unit_out /*[n_rows] or NULL*/, somhip_distortion_totals *totals);
int  somhip_distortion_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]);

/* ---- map sets: many maps of one shape, trained at once ---------------------------
 * What vfind does: N maps that share shape, data and schedule and differ only in their initial rows.  The online
 * algorithm on ONE small map is one launch per iteration and the launch is the cost (a 12x8x5 map is one workgroup of
 * a 256-CU chip).  A map set keeps every map on the device, row-major [n_maps][n_rows][dim]; training gives each map a
 * workgroup that holds it in LDS for a whole chunk of iterations (kernels/mapset.hpp), so a chunk is one launch however
 * many maps there are.  Every map comes out as somhip_som_train(batch 1) on a codebook of its rows leaves it, bit for
 * bit, traces included.
 * Shapes: hexa / rect maps whose LDS image, dim x (n_rows rounded up to 64) x 4 bytes, is at most 128 KiB (of the CU's
 * 160 KiB); somhip_mapset_create refuses larger ones with both numbers in its message, and somhip_debug_mapset_plan
 * answers the same question without a GPU.
 * A set whose engine was destroyed keeps a valid handle for somhip_mapset_destroy only (as codebooks do). */
typedef struct somhip_mapset somhip_mapset;
int  somhip_mapset_create(somhip_engine *e, const float *rows /*[n_maps][n_rows][dim]*/, int n_maps, int64_t n_rows,
                          int dim, int topol, int neigh, int xdim, int ydim, somhip_mapset **out);
int  somhip_mapset_download(somhip_mapset *ms, int first_map, int n_maps, float *rows);
int  somhip_mapset_upload(somhip_mapset *ms, int first_map, int n_maps, const float *rows);
void somhip_mapset_destroy(somhip_mapset *ms);
/* som_training (som_rout.c:556-671), batch 1, for every map of the set at once; p->batch must be 1.  start_iter, count
 * and data_first as in somhip_som_train: a run continued across calls equals one call.
 * trace_index / trace_diff: NULL or [n_maps][p->count], with -2 / -3 as somhip_som_train */
int  somhip_mapset_train(somhip_mapset *ms, somhip_dataset *ds, const somhip_som_params *p,
                         int32_t *trace_index, float *trace_diff);
/* find_winner_euc of data rows [first, first+count) against every map: index / diff / ret [n_maps][count] (ret may be
 * NULL); a sample with every component masked gives ret 0 and index -2, as somhip_find_winners */
int  somhip_mapset_winners(somhip_mapset *ms, somhip_dataset *ds, int64_t first, int64_t count,
                           int32_t *index, float *diff, int32_t *ret);
/* host arithmetic only, no GPU: out[0] = the shape fits, out[1] = threads per workgroup, out[2] = units per thread,
 * out[3] = LDS bytes per workgroup, out[4] = iterations per launch, out[5] = masked data, out[6..7] = 0
 * (out[1..3] are 0 where the shape does not fit) */
int  somhip_debug_mapset_plan(int64_t n_rows, int dim, int masked, int32_t out[8]);
/* HIP-event totals of the two set kernels since somhip_timing_reset, while somhip_timing_enable is on: [0] k_mapset_train,
 * [1] k_mapset_winners.  (The table of somhip_kernel_count / somhip_kernel_name is closed -- callers index it -- so these
 * two are not in it.) */
int  somhip_mapset_timing(somhip_engine *e, int64_t launches[2], double total_ms[2]);

/* ---- lvq1/olvq1/lvq2/lvq3_training (lvq_rout.c:498,584,702,808) --------------
 * kind = SOMHIP_LVQ1..LVQ3.  talpha (host, [n_rows], in/out) = OLVQ1's per-code
 * rates, initialised by the caller the way lvq_rout.c:614-627 does; `alpha` is also
 * OLVQ1's clamp (:671).  The result is the online (one sample at a time) result of the
 * reference, bit for bit; internally the loop runs as exact speculative batches (one
 * frozen-codebook scan per batch, samples certified and applied in order; see
 * kernels.hpp K6) unless SOMHIP_LVQ_ONLINE=1 or a row does not fit the on-chip cache
 * (dim > 2048), in which case every iteration is its own launch.
 * Masked data: distances and adapt_vector skip the sample's masked components
 * (lvq_pak.c:65-69, 179-186, 343-347), in the batched engine as in the per-iteration loop; a run that would visit a row with every component
 * masked is refused before anything is trained (the reference dereferences a NULL winner
 * there, lvq_rout.c:542-545).  The trace has knn entries per iteration (knn = 2 for
 * LVQ2/LVQ3, else 1). */
typedef struct somhip_lvq_params {
  int32_t kind;
  int64_t length;
  float   alpha;
  int32_t alpha_type;
  float   winlen;        /* -win     (lvq_rout.c:702) */
  float   epsilon;       /* -epsilon (lvq_rout.c:808) */
  int64_t start_iter, count, data_first;
} somhip_lvq_params;
int  somhip_lvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p,
                      float *talpha, int32_t *trace_index, float *trace_diff);
/* diagnostics (tests): the plan somhip_lvq_train would follow with these arguments (want_trace: a trace is asked for);
 * out[2], out[3], out[6], out[7] are also what somhip_lvq_batch_apply follows.  Host arithmetic only, no GPU work.
 * out[0] = engine (1 exact batched, 0 one launch per iteration), out[1] = the batched loop does not wait for the host
 * (0: every batch the careful way), out[2] = every batch is one component, out[3] = relation (*) over pairs by (0 the
 * masked direct-form kernel, 1 the MFMA Gram form, 2 the direct form), out[4] = masked data, out[5] = winners per
 * sample, out[6] = rows the walk's cache holds, out[7] = its dynamic LDS bytes */
int  somhip_debug_lvq_plan(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p, int want_trace,
                           int32_t out[8]);
/* diagnostics (tests): the front and the relation of ONE batch of the exact batched engine -- the top-8 scan, the
 * candidates' labels / rates, OLVQ1's rate bound, rho, relation (*) over all pairs, its components -- made exactly as
 * somhip_lvq_train makes them for the `count` (1..1024) iterations from p->start_iter on data rows data_first,
 * data_first + 1, ... (mod n), under the plan of the current environment (SOMHIP_LVQ_PAIRS_VALU and SOMHIP_LVQ_SERIAL
 * act as in training; p->count and p->data_first are not read).  Nothing is walked, trained or committed.  Host arrays:
 * keys [count][8] the candidate keys (all-ones: no entry), rho [count], xnorm [count] (the fp32 ||x_j||^2 the Gram form
 * uses), *amax the bound on |rate| used (< 0: unknown), adj [count][32] the adjacency bit rows (bit i % 32 of word i / 32
 * of row j: samples j and i are related; words from ceil(count / 32) on belong to no pair and are returned 0), *ncomp,
 * start [count + 1] (entries after start[ncomp]: -1) and comp_samples [count]: component c owns
 * comp_samples[start[c] .. start[c + 1]).  Under a one-component plan rho, xnorm and adj are not made and come back 0.
 * OLVQ1 takes its rates from somhip_lvq_rates_upload.  Refused with a message, before anything is launched: count outside
 * 1..1024, a plan that is not the batched engine's, a codebook or data set without labels, OLVQ1 without rates. */
int  somhip_debug_lvq_relation(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p, int64_t data_first,
                               int64_t count, uint64_t *keys, float *rho, float *xnorm, float *amax, uint32_t *adj,
                               int32_t *ncomp, int32_t *start, int32_t *comp_samples);
/* ... and the components stage alone on adjacency rows adj [count][32] the caller made (single != 0: one component, the
 * rows unread); ncomp, start [count + 1], comp_samples [count] as above */
int  somhip_debug_lvq_components(somhip_engine *e, const uint32_t *adj, int64_t count, int single, int32_t *ncomp,
                                 int32_t *start, int32_t *comp_samples);
/* out[0] = codebook rescans (batches) done by somhip_lvq_train so far, out[1] = samples,
 * out[2] / out[3] = batches cut short because a sample's candidate list was exhausted /
 * the on-chip row cache was full, out[4..7] = 100 MHz ticks the in-order kernel spent in
 * its phases (inputs, cached-row distances, decision, correction; summed over the components of a batch),
 * out[8] = independent components walked, out[9] = sum over the batches of the largest component's size
 * (the length of the longest serial walk), out[10] = (sample, 64-row group) pairs the exact top-k re-rank behind the
 * MFMA pre-filter evaluated, out[11] = 1 if the pair list of the last top-k search behind the pre-filter overflowed (its
 * samples then went through the one-wave exact re-rank), else 0 */
int  somhip_lvq_stats(somhip_engine *e, uint64_t out[12]);

/* ---- lininit's data passes (find_eigenvectors, som_rout.c:211-289) ----------------
 * sum[i] / count[i]: fp32 sum and number of the unmasked values of component i over all rows in
 * order (:243-254).  r[i*dim + j], j >= i: fp32 sum over the rows, in order, of
 * (x_i - mean_i) * (x_j - mean_j) for rows where neither component is masked (:266-284);
 * elements with j < i are left 0.  The eigenvector iteration itself is O(dim^2) host work. */
int  somhip_column_sums(somhip_dataset *ds, float *sum, int64_t *count);
int  somhip_centered_products(somhip_dataset *ds, const float *mean, float *r);

/* ---- randinit's data pass (randinit_codes, som_rout.c:98-131) --------------------
 * lo[i] / hi[i] / count[i]: smallest and largest unmasked value of component i over all rows, and their
 * number (count may be NULL).  The reference seeds its maximum with FLT_MIN and its minimum with FLT_MAX
 * (:108-111) -- apply that on the result; a component without data returns lo = FLT_MAX, hi = -FLT_MAX. */
int  somhip_column_minmax(somhip_dataset *ds, float *lo, float *hi, int64_t *count);

/* ---- find_qerror2 (som_rout.c:823-885; bubble_qerror :734-772, gaussian_qerror :775-818):
 * out[i] = sum over the neighbourhood of sample first+i's winner of (h *) d*d, d =
 * vector_dist_euc (lvq_pak.c:291-316), accumulated in fp32 in unit order exactly as the
 * reference does; ret[i] = 0 and out[i] = 0 for samples with every component masked (the
 * reference skips them, :858).  The caller adds out[] in data order (the reference's float
 * accumulator). */
int  somhip_qerror2(somhip_codebook *cb, somhip_dataset *ds, float radius, int64_t first,
                    int64_t count, float *out, int32_t *ret);

/* ---- two-phase mini-batch primitives (what somhip_som_train(batch>1) is made of;
 * exposed so a multi-GPU host can put its collective between them) -------------
 * keys: DEVICE array [count] of uint64 = (fp32 bits of squared distance << 32) |
 * global row index.  All distances are >= 0, so unsigned order == (distance, index)
 * order and an element-wise MIN across shards is exactly find_winner_euc over the
 * whole codebook, lowest index winning ties (lvq_pak.c:79).  "No winner in this shard"
 * is 0x7FFFFFFFFFFFFFFF, so every key is non-negative as int64 and a SIGNED 64-bit MIN
 * (all that torch.distributed / RCCL offer) orders them the same way.  A row at FLT_MAX or
 * beyond, or at NaN, beats nothing (lvq_pak.c:56): a sample with only such rows has that key too. */
int  somhip_batch_winner_keys(somhip_codebook *cb, somhip_dataset *ds, int64_t first,
                              int64_t count, uint64_t *dev_keys);
int  somhip_som_batch_update(somhip_codebook *cb, somhip_dataset *ds, const somhip_som_params *p,
                             int64_t batch_start_iter, int64_t count, int64_t data_first,
                             const uint64_t *dev_keys);
/* The same search over a ROW-SHARDED codebook with the pre-filter's bounds exchanged between the shards (find_winner_euc,
 * lvq_pak.c:41-96, over rows that live on several GPUs).  somhip_batch_winner_keys on a shard keeps every row group
 * within a window of the SHARD's smallest pre-filter value, so N shards together re-rank N times what one GPU would;
 * with the smallest bound of all shards in its place they re-rank what the whole codebook's search would:
 *     somhip_shard_winner_begin    level 1 of the pre-filter; dev_bound[count] (DEVICE floats) <- an upper bound on
 *                                  (squared distance to the nearest row of this shard) - ||x||^2; presets dev_keys
 *     host: all-reduce(MIN) of dev_bound as floats
 *     somhip_shard_winner_refine   level 2 for the groups within the exchanged bound; dev_bound <- the tighter bound
 *     host: all-reduce(MIN) of dev_bound
 *     somhip_shard_winner_finish   exact re-rank of the rows within the bound; dev_keys as somhip_batch_winner_keys
 *                                  (a shard that holds no candidate for a sample leaves 0x7FFFFFFFFFFFFFFF)
 *     host: all-reduce(MIN) of dev_keys, then somhip_som_batch_update
 * After the last all-reduce the keys are bit-identical to those of somhip_batch_winner_keys + all-reduce (the bounds only
 * remove rows that provably cannot win).  The three calls of one search share the engine's scratch memory: nothing else
 * may run on the engine between them (a call that is not the continuation of the search begun -- out of order, another
 * codebook, data set or range, a whole search in between -- is refused with an error).  somhip_shard_exchange_available: 1 if this shape takes the path (bf16 pre-filter,
 * ceil(ceil(dim / 4) / 2) a multiple of 4 -- dim 25..32, 57..64, 89..96, ... --, at least 64 rows, 225 <= count <= 65504,
 * no masks), else 0 -- every rank must take the same path, so a host
 * all-reduces the answer (MIN) once per run. */
int  somhip_shard_exchange_available(somhip_codebook *cb, somhip_dataset *ds, int64_t count);
int  somhip_shard_winner_begin(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                               uint64_t *dev_keys, float *dev_bound);
int  somhip_shard_winner_refine(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, float *dev_bound);
int  somhip_shard_winner_finish(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                                const float *dev_bound, uint64_t *dev_keys);
/* k-NN over a row-sharded codebook (the X2 exchange): dev_keys[count][knn] (knn = 1, 2, 4 or 8) =
 * this shard's knn best rows per sample, ascending; tag = global row index (SOMHIP_TIE_FIRST) or its
 * bitwise complement (SOMHIP_TIE_KNN: on equal distances the LATER row sorts first, lvq_pak.c:197).
 * Missing entries (shard smaller than knn) are all-ones.  All-gather the lists and keep the knn
 * smallest keys per sample: that is find_winner_knn (lvq_pak.c:152-221) over the whole codebook.
 * Masked data sets are accepted (exact direct-form scan, the sample's mask alone counts); a sample
 * with every component masked has distance 0 to every row here -- the reference finds no neighbour
 * for it (ret 0 of somhip_find_winners), so a host checks such rows itself. */
int  somhip_batch_topk_keys(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                            int knn, int tie, uint64_t *dev_keys);
/* The lists of all shards, all-gathered into dev_gathered[n_shards][count][knn] -> dev_keys[count][knn], the knn
 * smallest keys per sample, ascending: exactly the merge the comment above describes, on the device. */
int  somhip_merge_topk_keys(somhip_engine *e, const uint64_t *dev_gathered, int n_shards, int64_t count, int knn,
                            uint64_t *dev_keys);

/* ---- lvq1/olvq1/lvq2/lvq3_training (lvq_rout.c:498-916) over a ROW-SHARDED codebook -----------------------------
 * Every rank holds rows [row_offset, row_offset + n_rows) of the codebook (with their labels; OLVQ1: their rates,
 * somhip_lvq_rates_upload) and sees the same data.  One batch of count <= 1024 iterations is three calls, the
 * host's two collectives between them; the result is the reference's online result bit for bit, as with
 * somhip_lvq_train:
 *   1. somhip_batch_topk_keys(knn 8, tie = KNN for LVQ2/LVQ3 else FIRST)   this shard's 8 nearest rows per sample
 *        host: all-gather the lists, somhip_merge_topk_keys                 -> the frozen global top 8 (every rank)
 *   2. somhip_lvq_batch_candidates   labels / OLVQ1 rates of the 8 listed rows and tile copies of the `xrows`
 *        nearest ones, filled in for the rows this shard owns, zero elsewhere:
 *          dev_lab[count][8] int32, dev_ta[count][8] float (OLVQ1; else may be NULL),
 *          dev_rows[count][xrows][4 * ceil(dim / 4)] float
 *        host: all-reduce(SUM) of the three buffers as 32-bit INTEGERS (exact: every other rank adds 0)
 *   3. somhip_lvq_batch_apply   every rank walks the batch (kernels/lvq_batch.hpp: the walk is deterministic, so
 *        all ranks take the same decisions) and commits the corrected rows it owns.  *consumed <= count iterations
 *        were applied -- the same number on every rank; the next batch starts there.  A winner beyond the `xrows`
 *        exchanged rows ends the batch early (a larger xrows trades exchange volume for longer batches; 8 = never).
 * trace_index / trace_diff: as somhip_lvq_train, for the consumed iterations.
 * Masked data sets are accepted (every rank's data set carries the masks: the scan of step 1 and the walk of step 3
 * use the sample's mask); a batch that contains a row with every component masked is refused by
 * somhip_lvq_batch_apply with a message naming the row, as somhip_lvq_train refuses such a run. */
int  somhip_lvq_rates_upload(somhip_codebook *cb, const float *talpha);     /* [n_rows] local rows, lvq_rout.c:614-627 */
int  somhip_lvq_rates_download(somhip_codebook *cb, float *talpha);
int  somhip_lvq_batch_candidates(somhip_codebook *cb, int64_t count, int kind, const uint64_t *dev_keys, int xrows,
                                 int32_t *dev_lab, float *dev_ta, float *dev_rows);
int  somhip_lvq_batch_apply(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p,
                            int64_t batch_start_iter, int64_t count, int64_t data_first, const uint64_t *dev_keys,
                            const int32_t *dev_lab, const float *dev_ta, const float *dev_rows, int xrows,
                            int64_t *consumed, int32_t *trace_index, float *trace_diff);

/* ---- collectives for a C host with one process per GPU ---------------------------------------------
 * somhip_comm wraps an RCCL communicator (librccl.so is opened on first use, never linked): the all-reduce of packed
 * winner keys is ncclAllReduce(ncclUint64, ncclMin) enqueued on the engine's own stream between
 * somhip_batch_winner_keys and somhip_som_batch_update -- no host synchronisation in the step.
 *   rank 0: somhip_comm_unique_id(id)  ->  the host hands the 128 bytes to the other ranks (pipe, file, MPI, ...)
 *   all:    somhip_comm_create(engine, id, rank, world, &comm)
 * somhip_comm_create_sockets: the same operations over host sockets in a star around rank 0 (fds: rank 0 passes the
 * world-1 descriptors of ranks 1.., every other rank its one descriptor to rank 0) -- for rehearsals in which several
 * ranks share a GPU (RCCL refuses duplicate devices); each operation then synchronises and stages through the host.
 * allreduce_sum_u32 / allgather serve the LVQ exchange (candidate rows as integers; per-shard top-8 lists). */
typedef struct somhip_comm somhip_comm;
int  somhip_comm_unique_id(void *id128);
int  somhip_comm_create(somhip_engine *e, const void *id128, int rank, int world, somhip_comm **out);
int  somhip_comm_create_sockets(somhip_engine *e, int rank, int world, const int *fds, somhip_comm **out);
int  somhip_comm_allreduce_min_keys(somhip_comm *c, uint64_t *dev_keys, int64_t count);
int  somhip_comm_allreduce_min_f32(somhip_comm *c, float *dev_values, int64_t count);   /* the bounds of somhip_shard_winner_* */
int  somhip_comm_allreduce_sum_u32(somhip_comm *c, uint32_t *dev_words, int64_t count);
int  somhip_comm_allgather(somhip_comm *c, const void *dev_send, void *dev_recv, int64_t bytes_per_rank);
/* dev_buf of rank root to every rank's dev_buf: ncclBroadcast on the engine's stream, or through rank 0's star */
int  somhip_comm_broadcast(somhip_comm *c, void *dev_buf, int64_t bytes, int root);
void somhip_comm_destroy(somhip_comm *c);
/* The batch map (K8) with the DATA divided over the ranks: every rank holds the whole map (an ordinary codebook, the same
 * rows on every rank) and its own block of the data; p->first / p->n select rows of the block, and a rank whose block is
 * empty passes n == 0 (block is then not looked at).  Per epoch: (1) every rank runs the group stage -- the winner search,
 * the expensive part -- on its block at the same time; (2) for root = 0 .. G-1, rank root continues the sums and the q chain
 * (somhip_batchmap_accumulate's kernel) and the state blob is broadcast from it, so that after the last turn every rank
 * holds the full state; (3) rank r runs the combine for its ceil(ngroups / G) consecutive row groups; (4) the ranks
 * all-gather those groups' tiles.  Every rank ends every epoch with the same rows: bit for bit what somhip_som_batchmap
 * leaves on one GPU over the blocks concatenated in rank order, and the same qerror_out (asked for on every rank or on
 * none: the chain goes through all of them).  Refused before anything is launched: what somhip_som_batchmap refuses of the
 * codebook, the epochs, the radius and (where n > 0) the block, a communicator of another engine, and -- on every rank
 * alike, after one all-reduce of the counts -- blocks whose rows together number 2^32 or more.  An error later on (a peer
 * that went away) may leave this rank's rows part-way through an epoch; the state is closed and freed on every way out. */
int  somhip_som_batchmap_ranks(somhip_codebook *cb, somhip_dataset *block, const somhip_batchmap_params *p,
                               somhip_comm *c, float *qerror_out /*[count] or NULL*/);

/* ---- Sammon mapping of a codebook (SOM_PAK sammon.c) -------------------------------
 * The codebook is a whole one (no shard).  Mirrors carry no masks: a host whose codebook has masked components refuses
 * before it gets here (the tool and the reference differ there: vector_dist_euc would skip them).
 *
 * somhip_sammon_zero_pairs: the pairs of rows i < j whose distance dd(i, j) (vector_dist_euc, lvq_pak.c:291-316) is
 * 0.0 -- what remove_identicals (sammon.c:84-128) asks.  That is the computed distance, not equality of the rows: the
 * squares of small differences underflow.  pairs (may be NULL) has room for `cap` pairs {i, j}; *n_pairs is the number
 * found, also when it is larger than cap (the first cap pairs in (i, j) order are then not guaranteed: call again
 * with room for all).  The pairs returned are sorted by (i, j).
 *
 * somhip_sammon: rlen iterations of sammon.c:187-225 from the caller's initial table x[n_rows], y[n_rows] (in and
 * out), bit for bit.  mapping_error: NULL, or [rlen] for the error after every iteration (sammon.c:227-240); that one
 * number is summed in double by a tree where the reference adds in fp32 in sequence, so it is close, not bit-equal.
 * Refused: fewer than 2 rows (the reference writes NaNs), a shard, and a zero distance left in the codebook (the
 * reference would divide by it) -- remove those rows first.  The distance table is a full n_rows x n_rows fp32 matrix
 * in device memory; if it cannot be allocated the call fails with a message that says how large it is. */
int  somhip_sammon_zero_pairs(somhip_codebook *cb, uint32_t *pairs, int64_t cap, int64_t *n_pairs);
int  somhip_sammon(somhip_codebook *cb, int64_t rlen, float *x, float *y, double *mapping_error);

/* ---- within-class nearest neighbours of a data set (LVQ_PAK mindist / stddev / balance) ----
 * The inner loop of med_distances / min_distances (lvq_rout.c:280-491) over a data set that has labels
 * (somhip_dataset_create with labels, or somhip_dataset_generate with centres: the mixture ids):
 *   min_sq[r] = the smallest squared distance from row r to a LATER row of the same label -- the fp32 sum of
 *               vector_dist_euc (lvq_pak.c:291-316) before its root, bit for bit; a component masked in either row
 *               is skipped.  The distance itself is (float) sqrt((double) min_sq[r]): the root is monotone.
 *               +inf where no later row of the label is at a finite distance (the reference keeps FLT_MAX there)
 *   state[r]  = 0 no later row of that label, 1 min_sq[r] valid,
 *               2 some later row of the label shares no unmasked component with row r (vector_dist_euc returns -1
 *                 there, and -1 wins the reference's `dist < dissf`)
 * Both arrays are host memory, [n_rows].  Exact direct-form arithmetic on the vector ALU; work sum n_c^2 d / 2. */
int  somhip_class_nearest_later(somhip_dataset *ds, float *min_sq, int32_t *state);

/* ---- the U-matrix of a map (SOM_PAK umat: map.c calc_umatrix, average_umatrix, median_umatrix) ----
 * The distances between neighbouring model vectors of a whole hexa or rect map, the medians at the units' own
 * positions, the scaling to [0, 1] and the optional filters, bit for bit, from the rows as they are on the device now
 * (after training included); no data set and no host copy of the rows is involved.
 *   u       host, [uy][ux] floats with ux = 2 xdim - 1, uy = 2 ydim - 1: u[y * ux + x] = the reference's uvalue[x][y]
 *           after calc_umatrix, then average_umatrix (SOMHIP_UMAT_AVERAGE), then median_umatrix (SOMHIP_UMAT_MEDIAN)
 *   minmax  NULL, or the smallest and the largest entry before the scaling (map.c:474-485)
 * Refused before any launch: a codebook that is not a map, a shard (contiguous or interleaved), a side below 2 (the
 * reference reads outside its arrays there), unknown filter bits; after the reduction: max == min (the reference
 * divides by zero there). */
enum { SOMHIP_UMAT_AVERAGE = 1, SOMHIP_UMAT_MEDIAN = 2 };
int  somhip_umatrix(somhip_codebook *cb, int filters, float *u, double minmax[2]);

/* ---- grey-scaled component planes of a codebook (SOM_PAK planes: planes.c print_plane) ----
 * For the n_planes components from first_plane on, from the rows as they are on the device now, without a host copy
 * of the rows:
 *   lo, hi  NULL, or [n_planes]: minval and maxval of the component over all rows (planes.c:146-157).  Of rows that
 *           compare equal (+0.0 and -0.0) the first one's bits are kept, as the reference's comparisons keep them.
 *   grey    host, [n_planes][n_rows], plane-major: grey[j * n_rows + k] is the grey level of component first_plane + j
 *           of row k (the reference's row order), bit for bit
 *             (float)(0.05 + 0.9 * (double)(float)(p - minval) / (double)(float)(maxval - minval))
 *           and 0.5 where the float difference maxval - minval is zero (planes.c:172-176).
 * Any topology is taken.  A caller bounds what both sides hold at once by asking for the planes in windows.
 * Refused before any launch: null arguments, a codebook whose engine was destroyed, a shard (contiguous or
 * interleaved), n_planes < 1, a window that is not inside [0, dim).  Non-finite components: as in the reference,
 * minval starts at FLT_MAX and maxval at -FLT_MAX, so a NaN takes no part in either, +inf is never minval and -inf never
 * maxval (a column of +inf alone has lo = FLT_MAX, hi = +inf); the grey levels follow from those by the formula above. */
int  somhip_planes(somhip_codebook *cb, int first_plane, int n_planes, float *grey, float *lo, float *hi);

/* device scratch helpers for hosts without their own allocator */
int  somhip_device_alloc(somhip_engine *e, int64_t bytes, void **dev_ptr);
int  somhip_device_free(somhip_engine *e, void *dev_ptr);
int  somhip_copy_to_host(somhip_engine *e, void *host_dst, const void *dev_src, int64_t bytes);
int  somhip_copy_to_device(somhip_engine *e, void *dev_dst, const void *host_src, int64_t bytes);

/* ---- instrumentation ---------------------------------------------------------
 * Per-kernel launch statistics measured with HIP events on the engine's stream
 * (used by bench.py for the roofline line).  name = one of the kernel names
 * returned by somhip_kernel_name(i), i in [0, somhip_kernel_count()). */
int  somhip_timing_enable(somhip_engine *e, int on);
/* restrict the events to the kernels whose bit (1 << kernel id) is set; default all */
int  somhip_timing_select(somhip_engine *e, uint64_t kernel_mask);
int  somhip_timing_reset(somhip_engine *e);
int  somhip_kernel_count(void);
const char *somhip_kernel_name(int i);
int  somhip_timing_get(somhip_engine *e, int kernel, int64_t *launches, double *total_ms);

#ifdef __cplusplus
}
#endif

/* batch Robust Soft LVQ (K13): its entry points have a header of their own, which every user of this one gets */
#include "somhip_rslvq.h"
/* batch GLVQ (K9) over data in pieces and over the row blocks of ranks: somhip_glvq_begin / _accumulate / _finish / _end /
 * _state and somhip_glvq_train_ranks, likewise */
#include "somhip_glvq_pieces.h"
/* dense batch neural gas (K10d): somhip_ng_train_dense, neural gas over every rank of up to SOMHIP_NG_DENSE_MAX rows, likewise */
#include "somhip_ng_dense.h"
/* the batch map over data with missing values (K8m): somhip_som_batchmap_missing, its two stages and its five calls over
 * data in pieces, likewise */
#include "somhip_batchmap_missing.h"
#endif /* SOMHIP_H */
