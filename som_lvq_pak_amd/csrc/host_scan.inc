// host_scan.inc -- winner scans: exact scan, MFMA pre-filter + re-rank, top-k, k-NN / qerror2 / lininit entry points
// (included by somhip.hip: one translation unit, shared static helpers)

// ---------------------------------------------------------------------------------
// winner scans
// ---------------------------------------------------------------------------------
constexpr int SCAN_S = 32;     // samples per workgroup tile

static int check_pair(const somhip_codebook *cb, const somhip_dataset *ds, const char *who) {
  if (!cb || !ds) return fail("%s: null handle", who);
  if (!cb->e || !ds->e) return fail("%s: the engine of this handle was destroyed", who);
  if (cb->e != ds->e) return fail("%s: codebook and data belong to different engines", who);
  if (cb->v.d != ds->d)
    return fail("%s: code dimension (%d) != data dimension (%d)", who, cb->v.d, ds->d);   // som_rout.c:591-596
  return 0;
}

constexpr int64_t MFMA_MIN_SAMPLES = 32;

// Bound on |s~ + ||x||^2 - d| / (||x|| + ||c||)^2 (DESIGN.md section 4): fp32 MFMA GEMM form vs the
// reference's direct form, u = 2^-24, gamma_k = k u / (1 - k u):  2 * gamma_{d+2}.
// Split-bf16 form (kernels.hpp K2b): the dot product loses at most 3.1 * 2^-16 ||x|| ||c|| to the
// dropped lo*lo / residual terms and accumulates 3d exact products in fp32 -- bounded here with
// a factor 2 on the accumulation (no assumption on the matrix pipe's internal summation order or
// rounding mode beyond "error of a sum of k terms <= 2 gamma_k * sum |terms|"), sum |terms| <=
// 1.02 ||x|| ||c||.  The cn term and the direct-form term are as in the fp32 case.
// |s~ + ||x||^2 - d_ref| <= prod * ab + sq * (a + b)^2 for the distance GEMM in use (a = ||x||, b = ||c||, u = 2^-24,
// gamma_k = k u / (1 - k u), d_ref = the reference's direct-form fp32 sum):
//   split-bf16, three products (hi hi + hi lo + lo hi; every bf16 x bf16 product is exact in fp32):
//     fp32 accumulation of 3 d products in an order (and with an internal rounding) we do not know:  |dot~ - sum| <=
//       2 gamma_{3(d+2)} sum |p|,  sum |p| <= 1.01 ab;     dropped lo lo and split residuals: <= 1.55 2^-16 ab;
//     both enter s~ = cn - 2 dot twice                                   -> prod = 4.04 gamma_{3(d+2)} + 3.1 2^-16 + 2 u
//     cn = fl(sum c^2): gamma_{d+2} b^2;  d_ref: gamma_{d+2} d <= gamma_{d+2} (a + b)^2;  the final subtraction: u (a + b)^2
//                                                                         -> sq = 2 gamma_{d+2} + 2 u
//   The PRODUCT form matters: (a + b)^2 >= 4 ab, and more while the map is still bunched around the data's mean
//   (b ~ a / 3).  (Round 1 and most of round 2 charged everything to (a + b)^2: tau was 1.6 - 1.9 x wider, and the
//   exact re-rank looked at 20 rows per vector instead of ~11.)
//   fp32 MFMA scan mode: one exact-product sum of d terms -> everything in sq, as before.
static void prefilter_err3(const somhip_engine *e, int d, double *prod, double *sq) {
  const double u = 5.9604644775390625e-08;
  const double k = (d + 2) * u;
  const double gam = k / (1.0 - k);
  if (e->scan_mode == SOMHIP_SCAN_MFMA_BF16) {
    const double k3 = 3.0 * (d + 2) * u;
    *prod = 4.04 * (k3 / (1.0 - k3)) + 3.1 / 65536.0 + 2.0 * u;
    *sq = 2.0 * gam + 2.0 * u;
  } else {
    *prod = 0.0;
    *sq = 2.0 * gam;
  }
}

// Level 1 of the two-level pre-filter (kernels/prefilter_mfma.hpp K2c): ONE bf16 product, hi x hi.  With a = ||x||,
// b = ||c||, u = 2^-24, gamma = gamma_{d+2}:
//   <c,x> - <c_hi,x_hi> = <c_lo,x> + <c_hi,x_lo>,  |.| <= 2^-9 ab + (1 + 2^-9) 2^-9 ab <= 2^-8 (1 + 2^-8) ab
//                                                   (bf16 by round-to-nearest: |v - hi| <= 2^-9 |v|)
//   fp32 accumulation of d exact products, any order:   <= 2 gamma 1.01 ab
//   the norm term cn, the reference's direct-form sum, the final subtraction:  <= (2 gamma + u) (a + b)^2
// so |s~1 - s| <= prod * ab + sq * (a + b)^2 with the two coefficients below (s~ carries -2 <c,x>: the factor 2).
static void prefilter_err_l1(int d, double *prod, double *sq) {
  const double u = 5.9604644775390625e-08;
  const double k = (d + 2) * u;
  const double gam = k / (1.0 - k);
  *prod = 2.0 * ((1.0 / 256.0) * (1.0 + 1.0 / 256.0) + 2.02 * gam);
  *sq = 2.0 * gam + u;
}

// The route of a search, for every caller.  want: 1 = the nearest row, K (2, 4, 8) = the K nearest, 0 = bare pre-filter
//   9 .. SOMHIP_KNN_MAX = that many nearest rows by the wide k-NN route (K1w)
enum ScanRoute { ROUTE_MASKED, ROUTE_DIRECT, ROUTE_ONE_LEVEL, ROUTE_TWO_LEVEL, ROUTE_WIDE };
struct ScanPlan {
  ScanRoute route;
  int want, kth;       // kth: level 1's window above the smallest group minimum (1) or the LVQ_K0-th (k_group_kth)
  bool bf16, l1_ring;  // split-bf16 GEMMs (else fp32 MFMA); level 1 by the persistent ring kernel
  bool l1_wide;        // level 1 on 256 x 256 tiles (the ring kernel, k_dist_mfma_bf16_l1w16), else 128 x 256
  int64_t nsb, bpad;   // 32-sample tiles of the run, and the run padded to them
  int d8;              // 8-dim bf16 K-steps of a row
  bool by_group;       // top-K behind a pre-filter: exact re-rank filed by row group (k_topk_pairs_bygroup), else by pair
  bool l2_global;      // two levels: level 2's sample operand from global memory (k_dist_l2), else from LDS (k_dist_l2_lds)
  bool fused_gmin;     // two levels, nearest row: the per-sample minimum comes out of level 2 (else k_group_min)
  int64_t chunk;       // wide k-NN: samples per chunk (knn_wide_chunk)
};
// Wide k-NN: the samples of a chunk.  The distance matrix of a chunk, 4 * ngroups * 64 bytes per sample, stays within
// KNN_DIST_BYTES: whole sample tiles, at most 4096 samples, at least one tile.
constexpr int64_t KNN_DIST_BYTES = 256ll << 20;
static int64_t knn_wide_chunk(const somhip_codebook *cb) {
  const int64_t fit = KNN_DIST_BYTES / ((int64_t)sizeof(float) * cb->v.ngroups * WAVE) / SCAN_S * SCAN_S;
  return std::max<int64_t>(SCAN_S, std::min<int64_t>(4096, fit));
}
static ScanPlan scan_plan(const somhip_codebook *cb, const somhip_dataset *ds, int64_t count, int want) {
  const int64_t nsb = (count + SCAN_S - 1) / SCAN_S;
  ScanPlan p = {ROUTE_DIRECT, want, 1, cb->e->scan_mode == SOMHIP_SCAN_MFMA_BF16, false, false, nsb, nsb * SCAN_S, (cb->v.d4 + 1) / 2};
  if (want > 8) {                                  // masked or not, in every scan mode: exact, no pre-filter
    p.route = ROUTE_WIDE;
    p.chunk = knn_wide_chunk(cb);
    return p;
  }
  const bool run_ok = count >= MFMA_MIN_SAMPLES && count <= (int64_t)PAIR_MAX_COLS * 32;   // longer runs: the direct scan
  bool prefilter = cb->e->scan_mode != SOMHIP_SCAN_DIRECT;
  if (want == 1) prefilter = prefilter && run_ok && cb->v.n >= 64;
  else if (want > 1) {
    // big codebooks: bf16 pre-filter + exact re-rank of the surviving row groups (kernels.hpp K2k)
    prefilter = p.bf16 && run_ok && cb->v.n >= (getenv("SOMHIP_TOPK_MFMA") ? 64 : 4096);
    // two levels pay on big codebooks (100 000 x 1024: 0.52 -> 0.43 ms per 1024 samples); on 10 000 rows the
    // level-2 block costs more than the two products it saves (0.026 -> 0.049 ms)
    if (prefilter && want == LVQ_K0 && cb->v.ngroups >= 512 && !getenv("SOMHIP_TOPK_ONE_LEVEL")) p.kth = LVQ_K0;
  }
  // two-level form (K2c): bf16 mode, whole k-steps pairs, sample indices that fit 16 bits; behind it either the
  // re-rank of the nearest row (window above the smallest level-1 group minimum) or a top-K search (kth = K: window
  // above the K-th smallest -- a row of the true top K has level-1 value <= S_K + d1 <= (K-th smallest level-1 row
  // value) + 2 d1 <= (K-th smallest level-1 group minimum) + 2 d1; the groups left out keep their level-1 minimum,
  // which lies above S_K + d1 >= S_K + 3 d3: beyond the K-th smallest three-product minimum plus tau, so
  // k_topk_select never takes them and its K-th smallest is formed from exact three-product values).
  if (ds->d_mask) p.route = ROUTE_MASKED;
  else if (!prefilter) p.route = ROUTE_DIRECT;
  else if (p.bf16 && (want == 1 || p.kth > 1) && (p.d8 % 4) == 0 && nsb >= 8 && p.bpad <= 65535) p.route = ROUTE_TWO_LEVEL;
  else p.route = ROUTE_ONE_LEVEL;
  // level 1 as the persistent ring kernel: the wide tile's shape (>= 512 row groups), an even number of 32-dim K-steps
  // (a shard of a map has few row groups but the same long batches: the persistent kernel needs tiles, not rows -- at
  // least one 256 x 256 tile per CU)
  const int64_t l1_tiles = ((nsb + 7) / 8) * ((cb->v.ngroups + 3) / 4);
  p.l1_ring = p.route == ROUTE_TWO_LEVEL && (cb->v.ngroups >= 512 || l1_tiles >= 256) && (p.d8 % 8) == 0;
  p.l1_wide = cb->v.ngroups >= 512 || p.l1_ring;        // 256 x 256 tile: a third less L2 -> LDS traffic per MFMA
  // the re-rank behind a top-K pre-filter filed by row group when rows are whole float4s (64 KiB of LDS for the samples'
  // rows; a workgroup per group needs many groups to fill the chip)
  // (ngroups >= 512: on configs[2]'s 157 groups the by-group pass is faster than the pairs -- 100 against 117 us -- but the
  // step is not: 0.51 against 0.40 ms per 1024 iterations with the three extra launches and the lists' upkeep)
  const bool filtered = p.route == ROUTE_ONE_LEVEL || p.route == ROUTE_TWO_LEVEL;
  p.by_group = filtered && want > 1 && (cb->v.d & 3) == 0 && cb->v.d4 <= 256 && cb->v.ngroups >= 512 && !getenv("SOMHIP_TOPK_BYPAIR");
  p.l2_global = p.route == ROUTE_TWO_LEVEL && (p.d8 > 64 || getenv("SOMHIP_L2_GLOBAL") != nullptr);
  p.fused_gmin = p.route == ROUTE_TWO_LEVEL && want == 1 && !getenv("SOMHIP_NO_FUSED_GMIN");
  return p;
}
// (32-sample columns) x (chunks of about `per` row groups, whole 8s, at most 64): the passes over the group minima
// (chunks of 32 groups for k_l2_select, of 128 for k_rerank_select: profiles/r03_select_chunks.txt)
static dim3 group_chunks(int64_t ngroups, int64_t bpad, int64_t per, int64_t *chunk) {
  const int64_t nchunks = std::max<int64_t>(1, std::min<int64_t>(64, (ngroups + per - 1) / per));
  *chunk = ((ngroups + nchunks - 1) / nchunks + 7) / 8 * 8;
  return dim3((unsigned)(bpad / 32), (unsigned)((ngroups + *chunk - 1) / *chunk));
}

// MFMA pre-filter + exact re-rank (kernels.hpp K2/K2b/K2s/K2p/K2r/K2x) in stages over one binding of its buffers.
// The calls of a shard exchange find the state of the calls before them there: nothing else may run between them.
struct PrefilterBufs {
  float *tau, *wmin; uint64_t *wmask;     // per-sample window; per (group, sample) minimum and candidate mask
  void *xt; uint4 *xhi, *xlo, *xrow;      // tiles: fp32 xt[sb][q][32][4] or bf16 hi | lo [sb][kb][32][8]; xrow: sample-major
  uint32_t *gmin, *gcount, *colcount, *paircount;            // re-rank counters (preset in pf_prepare: rerank_presets)
  float *tau1; uint32_t *gmin1, *l2cnt; uint16_t *l2list;   // two levels: level 1's window and minimum, level 2's lists
  uint4 *l2out;                           // two levels, nearest row: level 2's (mask, minimum) per list slot, else null
  float *xw;                              // shard exchange: delta1, max(delta1, 3 delta3), delta3 per sample
};
static int bind_prefilter(somhip_codebook *cb, const ScanPlan &p, bool exchange, PrefilterBufs *b) {
  somhip_engine *e = cb->e;
  const int64_t bpad = p.bpad, ng = cb->v.ngroups;
  if (!cb->d_cn) {
    HIPCHK(hipMalloc((void **)&cb->d_cn, sizeof(float) * (size_t)ng * WAVE));
    HIPCHK(hipMalloc((void **)&cb->d_cnmax, 2 * sizeof(unsigned int)));      // two words in turn (pf_prepare)
    HIPCHK(hipMemsetAsync(cb->d_cnmax, 0, 2 * sizeof(unsigned int), e->stream));
    cb->cnmax_sel = 0;
    cb->cnmax_clean = true;
  }
  if (p.bf16 && !cb->d_chi) {
    HIPCHK(hipMalloc((void **)&cb->d_chi, sizeof(uint4) * (size_t)ng * p.d8 * WAVE));
    HIPCHK(hipMalloc((void **)&cb->d_clo, sizeof(uint4) * (size_t)ng * p.d8 * WAVE));
  }
  *b = PrefilterBufs{};
  CHK(scratch(e, SLOT_TAU, (size_t)bpad, &b->tau));
  CHK(scratch(e, SLOT_WMIN, (size_t)ng * bpad, &b->wmin));
  CHK(scratch(e, SLOT_WMASK, (size_t)ng * bpad, &b->wmask));
  const size_t xt_bytes = p.bf16 ? 2 * sizeof(uint4) * (size_t)p.nsb * p.d8 * 32 : sizeof(float4) * (size_t)p.nsb * cb->v.d4 * SCAN_S;
  CHK(engine_scratch(e, SLOT_SAMPLES, xt_bytes, &b->xt));
  b->xhi = (uint4 *)b->xt;
  b->xlo = b->xhi + (size_t)p.nsb * p.d8 * 32;
  CHK(scratch(e, SLOT_RERANK_COUNT, 2 * (size_t)bpad + 4 * (size_t)(bpad / 32), &b->gmin));
  b->gcount = b->gmin + bpad;
  b->colcount = b->gcount + bpad;
  b->paircount = reinterpret_cast<uint32_t *>(e->d_stats + STAT_PAIR_OVERFLOW);   // stays 0 unless a segment overflows
  if (exchange) CHK(scratch(e, SLOT_XBOUND, 3 * (size_t)bpad, &b->xw));
  if (p.route == ROUTE_TWO_LEVEL) {
    CHK(scratch(e, SLOT_SAMPLE_ROWS, xt_bytes / sizeof(uint4), &b->xrow));      // (two levels: bf16 tiles)
    CHK(scratch(e, SLOT_L2_STATE, 2 * (size_t)bpad + (size_t)ng, &b->tau1));    // 32-bit words: tau1 | gmin1 | l2cnt
    CHK(scratch(e, SLOT_L2_LIST, (size_t)ng * bpad, &b->l2list));
    if (p.want == 1) CHK(scratch(e, SLOT_L2_OUT, (size_t)ng * bpad, &b->l2out));   // (top-K, LVQ: nothing reads it)
    b->gmin1 = reinterpret_cast<uint32_t *>(b->tau1 + bpad);
    b->l2cnt = b->gmin1 + bpad;
  }
  return 0;
}
// prepare: the codebook's norms or bf16 split, the sample tiles, the windows and the re-rank's presets.  The windows need
// the codebook's largest norm: on the bf16 route the codebook pass runs first and k_pack_samples_bf16 forms the windows
// and the presets from the rows it packs; on the fp32 route k_sample_tau does, behind k_row_norms.
// d_keys: the nearest-row keys it presets (nullptr: top-K or bare pre-filter), as INT64_MAX under nonneg_keys (above
// every real key, and what a signed MIN all-reduce needs -- saves somhip_batch_winner_keys a pass over the keys)
static int pf_prepare(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, const ScanPlan &p,
                      const PrefilterBufs &b, uint64_t *d_keys, bool nonneg_keys) {
  somhip_engine *e = cb->e;
  const bool two = p.route == ROUTE_TWO_LEVEL;
  const int d8 = p.d8;
  // the lo tiles are read by the one-level GEMMs and by level 2 from global memory (k_dist_l2); level 2 in LDS takes both
  // pieces of a sample from xrow, and level 1 reads the hi tiles only
  const bool pack_lo = !two || p.l2_global;
  // the bf16 tiles and norms of an unchanged codebook are reused (read-only scans chunk by chunk; the LVQ engine
  // re-splits exactly the rows it corrected); every writer of the rows clears the flag
  const bool prep_was_current = p.bf16 && cb->prep_valid;
  const RerankInit rinit = {d_keys, b.gmin, b.paircount, p.bpad, (int)(p.bpad / 32), nonneg_keys ? 0x7FFFFFFFFFFFFFFFull : KEY_NONE,
                            b.gmin1, b.l2cnt, two ? cb->v.ngroups : 0};
  double l1_prod = 0.0, l1_sq = 0.0, err_prod = 0.0, err_sq = 0.0;
  prefilter_err3(e, ds->d, &err_prod, &err_sq);
  if (two) prefilter_err_l1(ds->d, &l1_prod, &l1_sq);
  // the word the codebook pass folds its largest norm into must be zero before it.  Two words in turn: the bf16 pack
  // kernel, the last reader of this search's word, clears the word of the NEXT search -- no launch of its own for that.
  // (cnmax_clean: this search's word is known to be zero; not so after an fp32 search or an error)
  unsigned int *cnmax = cb->d_cnmax + cb->cnmax_sel;
  if (!p.bf16 || !cb->cnmax_clean) HIPCHK(hipMemsetAsync(cnmax, 0, sizeof(unsigned int), e->stream));
  cb->cnmax_clean = false;
  if (!p.bf16)
    CHK(LAUNCH_TIMED(e, KID_PACK_SAMPLES, k_pack_samples<SCAN_S>, dim3((unsigned)p.nsb), dim3(256), 0, ds->d_rows, ds->n, ds->d, cb->v.d4, first, count,
        (float4 *)b.xt));
  {
    LaunchTimer t(e, KID_NORMS);
    if (prep_was_current) {
      // tiles and norms are current (unchanged codebook, or the LVQ engine re-split the rows it corrected): only the maximum is due
      CHK(LAUNCH(e, k_max_norm, dim3(64), dim3(256), 0, cb->v, cb->d_cn, cnmax));
    } else if (p.bf16) {
      // with the tiles a row-major copy of the rows for the exact re-rank of single rows (k_rerank_pairs), where that
      // kernel will run behind this pre-filter on a long enough run (a shard of a map included)
      // (the copy saves 36 us of re-rank per 4096 vectors at 65536 x 512: from 8192 vectors per run on)
      const bool want_rm = p.want == 1 && (cb->v.d & 3) == 0 && cb->v.ngroups >= 64 && count >= 8192;
      if (want_rm && !cb->d_rowmajor) HIPCHK(hipMalloc((void **)&cb->d_rowmajor, sizeof(float) * (size_t)cb->v.ngroups * WAVE * cb->v.d));
      const int prep_threads = d8 >= 16 ? 1024 : d8 >= 4 ? 256 : 64;
      if (want_rm) {
        CHK(raise_lds_limit(e, LDS_PREP_ROWMAJOR, (const void *)k_prep_codes_bf16<true>, PREP_RM_LDS(16)));
        CHK(LAUNCH(e, k_prep_codes_bf16<true>, dim3((unsigned)cb->v.ngroups), dim3(prep_threads), PREP_RM_LDS(prep_threads / 64), cb->v, d8, cb->d_cn,
            cnmax, cb->d_chi, cb->d_clo, cb->d_rowmajor));
      } else
        CHK(LAUNCH(e, k_prep_codes_bf16<false>, dim3((unsigned)cb->v.ngroups), dim3(prep_threads), 0, cb->v, d8, cb->d_cn, cnmax, cb->d_chi,
            cb->d_clo, nullptr));
      cb->prep_valid = true;
      cb->rowmajor_valid = want_rm;
    } else {
      CHK(LAUNCH(e, k_row_norms, dim3((unsigned)((cb->v.ngroups + 3) / 4)), dim3(256), 0, cb->v, cb->d_cn, cnmax));
      CHK(LAUNCH(e, k_sample_tau, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, ds->d_rows, ds->n, ds->d, first, count, cnmax, err_prod, err_sq,
          b.tau, rinit, l1_prod, l1_sq, b.tau1, b.xw));
    }
  }
  if (p.bf16) {
    CHK(LAUNCH_TIMED(e, KID_PACK_SAMPLES, k_pack_samples_bf16, dim3((unsigned)p.nsb), dim3(PACK_THREADS), 0, ds->d_rows, ds->n, ds->d, d8, first, count,
        b.xhi, pack_lo ? b.xlo : nullptr, cb->d_cnmax + (cb->cnmax_sel ^ 1), b.xrow, cnmax, TauCoef{err_prod, err_sq, l1_prod, l1_sq}, b.tau, b.tau1,
        b.xw, rinit));
    cb->cnmax_sel ^= 1;
    cb->cnmax_clean = true;
  }
  return 0;
}
// level 1 (K2c): one bf16 product per (group, sample); per sample the smallest group minimum (k_group_min or the ring
// kernel's epilogue) or the K-th smallest (k_group_kth).  xbound (shard exchange) <- smallest level-1 value + delta1.
static int pf_level1(somhip_codebook *cb, int64_t count, const ScanPlan &p, const PrefilterBufs &b, float *xbound) {
  somhip_engine *e = cb->e;
  const int64_t ng = cb->v.ngroups, nsb = p.nsb;
  const bool l1_ring_gmin = p.l1_ring && p.kth != LVQ_K0;
  {
    LaunchTimer t(e, KID_DIST_MFMA_BF16);
    if (p.l1_wide) {
      dim3 gridw((unsigned)((nsb + 7) / 8), (unsigned)((ng + 3) / 4));
      if (p.l1_ring) {
        // persistent form over an LDS ring (kernels/prefilter_l1_ring.hpp): one workgroup per CU, a multiple of 8 of them
        CHK(raise_lds_limit(e, LDS_L1_RING, (const void *)k_dist_mfma_bf16_l1r, L1R_LDS_BYTES));
        if (!e->n_cus) {
          int v = 0;
          HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, e->device));
          e->n_cus = v > 0 ? v : 256;
        }
        int nwg = e->n_cus >= 8 ? e->n_cus / 8 * 8 : e->n_cus;
        const int64_t ntiles = (int64_t)gridw.x * gridw.y;
        if (ntiles < nwg) nwg = (int)ntiles;
        CHK(LAUNCH(e, k_dist_mfma_bf16_l1r, dim3((unsigned)nwg), dim3(512), L1R_LDS_BYTES, cb->v, p.d8, cb->d_chi, b.xhi, cb->d_cn, p.bpad, b.wmin,
            l1_ring_gmin ? b.gmin1 : nullptr, (int)gridw.x, (int)gridw.y));
      } else
        CHK(LAUNCH(e, (k_dist_mfma_bf16_l1w16<4>), dim3(gridw.x * gridw.y), dim3(512), 0, cb->v, p.d8, cb->d_chi, b.xhi, cb->d_cn, p.bpad, b.wmin,
            (int)gridw.x, (int)gridw.y));
    } else {
      dim3 gridw((unsigned)((nsb + 7) / 8), (unsigned)((ng + 1) / 2));
      CHK(LAUNCH(e, (k_dist_mfma_bf16_l1<4>), gridw, dim3(256), 0, cb->v, p.d8, cb->d_chi, b.xhi, cb->d_cn, p.bpad, b.wmin));
    }
  }
  LaunchTimer t(e, KID_DIST_L2);
  int64_t chunk;
  const dim3 sgrid = group_chunks(ng, p.bpad, 32, &chunk);
  if (p.kth == LVQ_K0)
    CHK(LAUNCH(e, k_group_kth<LVQ_K0>, dim3((unsigned)(p.bpad / 32)), dim3(1024), 0, ng, p.bpad, b.wmin, b.gmin1));
  else if (!l1_ring_gmin)                            // (the ring kernel's epilogue has folded the minima into gmin1 itself)
    CHK(LAUNCH(e, k_group_min, sgrid, dim3(256), 0, ng, p.bpad, chunk, b.wmin, b.gmin1));
  if (xbound)
    CHK(LAUNCH(e, k_shard_bound, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, count, b.gmin1, b.xw, xbound));
  return 0;
}
// level 2 (K2c): the three-product split for the groups level 1 keeps.  fused_gmin: the per-sample minimum behind it
// comes out of the level-2 kernel itself (an atomicMin per (group, sample) it covers) instead of a pass over the whole
// wmin matrix (k_group_min: 21 us per 32768 vectors and a launch).  xbound (shard exchange): in, the MIN of the
// shards' level-1 bounds (window max(delta1, 3 delta3)); out, the smallest kept three-product value + delta3.
static int pf_level2(somhip_codebook *cb, int64_t count, const ScanPlan &p, const PrefilterBufs &b, bool fused_gmin, float *xbound) {
  somhip_engine *e = cb->e;
  const int64_t ng = cb->v.ngroups, bpad = p.bpad;
  const int d8 = p.d8;
  int64_t chunk;
  const dim3 sgrid = group_chunks(ng, bpad, 32, &chunk);
  // (a workgroup: 1024 samples x a chunk of groups)
  CHK(LAUNCH_TIMED(e, KID_L2_SELECT, k_l2_select, dim3((unsigned)((bpad + 1023) / 1024), sgrid.y), dim3(256), 0, ng, count, bpad, chunk, b.wmin, b.gmin1,
      xbound ? b.xw + bpad : b.tau1, b.l2cnt, b.l2list, xbound ? b.wmin : nullptr, xbound));
  {
    LaunchTimer t(e, KID_DIST_L2);
    uint32_t *l2_gmin = fused_gmin ? b.gmin : nullptr;
    if (!p.l2_global) {
      const size_t a_bytes = sizeof(uint4) * 2 * (size_t)d8 * 64;
      CHK(raise_lds_limit(e, LDS_DIST_L2, (const void *)k_dist_l2_lds, 128 * 1024));
      CHK(LAUNCH(e, k_dist_l2_lds, dim3((unsigned)ng, 4), dim3(64 * L2_WAVES), a_bytes, cb->v, d8, cb->d_chi, cb->d_clo, b.xrow, cb->d_cn, b.tau,
          bpad, b.l2cnt, b.l2list, b.wmin, b.wmask, e->d_stats + STAT_L2_PAIRS, l2_gmin, b.l2out));
    } else
      CHK(LAUNCH(e, k_dist_l2, dim3((unsigned)ng, 8), dim3(256), 0, cb->v, d8, cb->d_chi, cb->d_clo, b.xhi, b.xlo, cb->d_cn, b.tau, bpad, b.l2cnt,
          b.l2list, b.wmin, b.wmask, e->d_stats + STAT_L2_PAIRS, b.xrow, l2_gmin, b.l2out));
  }
  if (xbound) {
    LaunchTimer t(e, KID_RERANK_SELECT);
    if (!fused_gmin) CHK(LAUNCH(e, k_group_min, sgrid, dim3(256), 0, ng, bpad, chunk, b.wmin, b.gmin));
    CHK(LAUNCH(e, k_shard_bound, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, count, b.gmin, b.xw + 2 * bpad, xbound));
  }
  return 0;
}
// one level: the distance GEMM of every (group, sample), fp32 or three-product bf16
static int pf_one_level(somhip_codebook *cb, int64_t count, const ScanPlan &p, const PrefilterBufs &b) {
  somhip_engine *e = cb->e;
  const int64_t nsb = p.nsb, ng = cb->v.ngroups;
  LaunchTimer t(e, p.bf16 ? KID_DIST_MFMA_BF16 : KID_DIST_MFMA);
  dim3 grid((unsigned)((nsb + 3) / 4), (unsigned)((ng + 1) / 2));
  if (p.bf16) {
    const bool wide = (p.d8 % 2) == 0 && nsb >= 8;
    if (wide) grid = dim3((unsigned)((nsb + 7) / 8), (unsigned)((ng + 1) / 2));
    auto kern = wide ? k_dist_mfma_bf16_wide<2> : (p.d8 % 4) == 0 ? k_dist_mfma_bf16_dma<4, 2> : k_dist_mfma_bf16;
    return launch(e, "k_dist_mfma_bf16", kern, grid, dim3(256), 0, cb->v, p.d8, cb->d_chi, cb->d_clo, b.xhi, b.xlo, cb->d_cn, b.tau, count, p.bpad, b.wmin,
                  b.wmask);
  }
  return LAUNCH(e, k_dist_mfma, grid, dim3(256), 0, cb->v, (const float4 *)b.xt, cb->d_cn, b.tau, count, p.bpad, b.wmin, b.wmask);
}
// the pre-filter of a whole search: prepare -> level 1 -> level 2, or prepare -> one level
static int pf_filter(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, const ScanPlan &p,
                     PrefilterBufs *b, uint64_t *d_keys, bool nonneg_keys, bool fused_gmin) {
  cb->e->xc_phase = XC_NONE;                       // a whole search takes the scratch of an exchanged one under way
  CHK(bind_prefilter(cb, p, false, b));
  CHK(pf_prepare(cb, ds, first, count, p, *b, d_keys, nonneg_keys));
  if (p.route == ROUTE_ONE_LEVEL) return pf_one_level(cb, count, p, *b);
  CHK(pf_level1(cb, count, p, *b, nullptr));
  return pf_level2(cb, count, p, *b, fused_gmin, nullptr);
}
// the nearest-row re-rank's pair list (SLOT_PAIRS): a segment of cap_col pairs per 32-sample column, cap pairs in all
struct RerankPairs { uint2 *pairs; uint32_t ncols, cap_col, cap; };
static int bind_rerank_pairs(somhip_engine *e, int64_t bpad, RerankPairs *r) {
  r->ncols = (uint32_t)(bpad / 32);
  r->cap_col = 16384;   // 512 per sample on average; a full segment -> K2r
  r->cap = (uint32_t)std::min<int64_t>((int64_t)r->ncols * r->cap_col, 0x7FFFFFF0);
  return scratch(e, SLOT_PAIRS, (size_t)r->ncols * r->cap_col + 2, &r->pairs);   // (16 spare bytes)
}
// the nearest-row re-rank: row-granular pairs for the usual few candidates (a segment per 32-sample column), k_rerank
// for flagged samples.  gmin_ready: the per-sample minimum is formed (else k_group_min).  xbound (shard exchange): the
// rows of the groups whose three-product minimum is <= (MIN over the shards of their bounds) + delta3.
// from_lists: the selection walks level 2's lists (k_rerank_select_lists; two levels only) instead of the whole wmin matrix
static int pf_rerank(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, const ScanPlan &p,
                     const PrefilterBufs &b, uint64_t *d_keys, bool gmin_ready, const float *xbound, bool from_lists) {
  somhip_engine *e = cb->e;
  const int64_t ng = cb->v.ngroups, bpad = p.bpad;
  RerankPairs pl;
  CHK(bind_rerank_pairs(e, bpad, &pl));
  {
    int64_t chunk;
    const dim3 sgrid = group_chunks(ng, bpad, 128, &chunk);
    LaunchTimer t(e, KID_RERANK_SELECT);
    if (!gmin_ready)
      CHK(LAUNCH(e, k_group_min, sgrid, dim3(256), 0, ng, bpad, chunk, b.wmin, b.gmin));
    const float *win = xbound ? b.xw + 2 * bpad : b.tau;
    if (from_lists && !b.l2out) return fail("pf_rerank: no level-2 results in list order for this search");
    if (from_lists)
      CHK(LAUNCH(e, k_rerank_select_lists, dim3((unsigned)ng, 4), dim3(256), 0, cb->v, count, bpad, b.l2cnt, b.l2list, b.l2out, win, b.gmin, b.gcount,
          pl.cap, pl.cap_col, pl.pairs, b.colcount, b.paircount, xbound));
    else
      CHK(LAUNCH(e, k_rerank_select, sgrid, dim3(256), 0, cb->v, count, bpad, chunk, b.wmin, b.wmask, win, b.gmin, b.gcount, pl.cap, pl.cap_col,
          pl.pairs, b.colcount, b.paircount, e->d_stats, xbound));
  }
  CHK(LAUNCH_TIMED(e, KID_RERANK_PAIRS, k_rerank_pairs, dim3(4096), dim3(256), 0, cb->v, ds->d_rows, ds->n, first, pl.cap, pl.cap_col, (int)pl.ncols,
      pl.pairs, b.colcount, b.paircount, d_keys, e->d_stats, p.bf16 && cb->prep_valid && cb->rowmajor_valid ? cb->d_rowmajor : nullptr));
  return LAUNCH_TIMED(e, KID_RERANK, k_rerank, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, cb->v, ds->d_rows, ds->n, first, count, bpad, b.wmin,
                      b.wmask, b.tau, b.paircount, pl.cap, d_keys, e->d_stats);
}
// the direct scan (K1): packed sample tiles against every row group; keys (top-1) or per-block top-K lists in part
template <int K>
static int scan_exact(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, const ScanPlan &p,
                      int tie_knn, uint64_t *keys, uint64_t *part) {
  somhip_engine *e = cb->e;
  float4 *xt;
  CHK(scratch(e, SLOT_SAMPLES, (size_t)p.nsb * cb->v.d4 * SCAN_S, &xt));
  CHK(LAUNCH_TIMED(e, KID_PACK_SAMPLES, k_pack_samples<SCAN_S>, dim3((unsigned)p.nsb), dim3(256), 0, ds->d_rows, ds->n, ds->d, cb->v.d4, first, count,
      xt));
  dim3 grid((unsigned)p.nsb, (unsigned)((cb->v.ngroups + 3) / 4));
  return LAUNCH_TIMED(e, KID_SCAN_EXACT, (k_scan_exact<SCAN_S, 1, K>), grid, dim3(256), 0, cb->v, xt, count, tie_knn, keys, part);
}
// masked samples (K1m / K1mk), one launch column each: column(offset, first sample, columns), 0 or an error, per 32768 (grid.y limit)
template <class Launch>
static int masked_columns(somhip_engine *e, const somhip_dataset *ds, int64_t first, int64_t count, Launch column) {
  for (int64_t off = 0; off < count; off += 32768) {
    const int64_t c = std::min<int64_t>(32768, count - off);
    LaunchTimer t(e, KID_SCAN_MASKED);
    CHK(column(off, (first + off) % ds->n, c));
  }
  return 0;
}
// keys[count] <- exact nearest row per sample, FIRST tie rule, local shard
static int scan_keys_top1(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                          uint64_t *d_keys, bool *nonneg_keys = nullptr) {
  somhip_engine *e = cb->e;
  const ScanPlan p = scan_plan(cb, ds, count, 1);
  if (p.route == ROUTE_MASKED || p.route == ROUTE_DIRECT)
    HIPCHK(hipMemsetAsync(d_keys, 0xFF, sizeof(uint64_t) * (size_t)count, e->stream));   // (else pf_prepare presets them)
  if (p.route == ROUTE_MASKED)
    return masked_columns(e, ds, first, count, [&](int64_t off, int64_t f, int64_t c) {
      return LAUNCH(e, k_scan_masked, dim3((unsigned)((cb->v.ngroups + 3) / 4), (unsigned)c), dim3(256), 0, cb->v, ds->d_rows, ds->d_mask, ds->n, f, c,
                    0, d_keys + off);
    });
  e->samples_searched += (uint64_t)count;
  if (p.route == ROUTE_DIRECT) return scan_exact<1>(cb, ds, first, count, p, 0, d_keys, (uint64_t *)nullptr);
  if (nonneg_keys) *nonneg_keys = true;
  PrefilterBufs b;
  CHK(pf_filter(cb, ds, first, count, p, &b, d_keys, nonneg_keys != nullptr, p.fused_gmin));
  return pf_rerank(cb, ds, first, count, p, b, d_keys, p.fused_gmin, nullptr, p.route == ROUTE_TWO_LEVEL);
}
// the by-group top-K re-rank's buffers, carved from SLOT_TOPK_GROUPS with the counts and the pass counter zeroed:
// [lists of the groups][their counts][the pass counter, padded][the passes: at most one per filed sample]
struct TopkGroupBufs { uint2 *glist; uint32_t *gcnt, *wcount; uint2 *work; };
static int bind_topk_groups(somhip_engine *e, int64_t ngroups, uint32_t cap_g, uint32_t cap, TopkGroupBufs *g) {
  const size_t words = (size_t)ngroups + 4 + (ngroups & 1);   // counts and counter, padded to whole uint2s
  void *p;
  CHK(engine_scratch(e, SLOT_TOPK_GROUPS, sizeof(uint2) * (size_t)ngroups * cap_g + sizeof(uint32_t) * words + sizeof(uint2) * (size_t)cap, &p));
  g->glist = (uint2 *)p;
  g->gcnt = reinterpret_cast<uint32_t *>(g->glist + (size_t)ngroups * cap_g);
  g->wcount = g->gcnt + ngroups;
  g->work = reinterpret_cast<uint2 *>(g->gcnt + words);
  HIPCHK(hipMemsetAsync(g->gcnt, 0, sizeof(uint32_t) * ((size_t)ngroups + 4), e->stream));
  return 0;
}
template <int K>
static int scan_keys_topk(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                          uint64_t *d_keys /*[count][K]*/, int tie_knn = 1) {
  somhip_engine *e = cb->e;
  const ScanPlan p = scan_plan(cb, ds, count, K);
  if (p.route == ROUTE_MASKED || p.route == ROUTE_DIRECT) {
    const int nblk = (int)((cb->v.ngroups + 3) / 4);
    uint64_t *part;
    CHK(scratch(e, SLOT_PARTIAL, (size_t)count * nblk * K, &part));
    if (p.route == ROUTE_MASKED)
      CHK(masked_columns(e, ds, first, count, [&](int64_t off, int64_t f, int64_t c) {
        return LAUNCH(e, k_scan_masked_topk<K>, dim3((unsigned)nblk, (unsigned)c), dim3(256), 0, cb->v, ds->d_rows, ds->d_mask, ds->n, f, tie_knn,
                      part + (size_t)off * nblk * K);
      }));
    else
      CHK(scan_exact<K>(cb, ds, first, count, p, tie_knn, (uint64_t *)nullptr, part));
    return LAUNCH_TIMED(e, KID_MERGE_TOPK, k_merge_topk<K>, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, part, nblk, count, d_keys);
  }
  PrefilterBufs b;
  CHK(pf_filter(cb, ds, first, count, p, &b, nullptr, false, false));
  // pair-parallel re-rank (three launches); the one-wave-per-sample kernel only if the list overflows
  const uint32_t cap = (uint32_t)std::min<int64_t>(count * 128 + 4096, 0x3FFFFFF0);
  uint2 *dpairs; TopkSpan *dspan; uint64_t *dpart;
  CHK(scratch(e, SLOT_PAIRS, (size_t)cap, &dpairs));
  CHK(scratch(e, SLOT_PARTIAL, (size_t)cap * K, &dpart));
  CHK(scratch(e, SLOT_TOPK_SPAN, (size_t)count + 2, &dspan));   // (16 spare bytes)
  uint32_t *dcounter = reinterpret_cast<uint32_t *>(e->d_stats + STAT_TOPK_LIST);
  HIPCHK(hipMemsetAsync(dcounter, 0, 2 * sizeof(uint32_t), e->stream));
  LaunchTimer t(e, KID_RERANK);
  // pairs filed by row group (scan_plan: by_group): the group's tile is then streamed once per four samples
  const bool by_group = p.by_group;
  // room per group: every sample of the run (a sample is filed at most once per group) unless that is too much memory
  // (then a crowded group sends the run to the overflow path)
  const uint32_t cap_g = (uint64_t)cb->v.ngroups * (uint64_t)count <= (8ull << 20)
                             ? (uint32_t)count : (uint32_t)std::max<uint64_t>(64, (8ull << 20) / (uint64_t)cb->v.ngroups);
  TopkGroupBufs g{};
  if (by_group) CHK(bind_topk_groups(e, cb->v.ngroups, cap_g, cap, &g));
  CHK(LAUNCH(e, k_topk_select<K>, dim3((unsigned)((count + TOPK_NB - 1) / TOPK_NB)), dim3(1024), 0, cb->v, count, p.bpad, b.wmin, b.tau, cap, dpairs,
      dspan, dcounter, g.gcnt, g.glist, cap_g));
  if (by_group) {
    CHK(LAUNCH(e, k_topk_worklist<4>, dim3((unsigned)std::min<int64_t>((cb->v.ngroups + 255) / 256, 256)), dim3(256), 0, cb->v.ngroups, g.gcnt, cap_g,
        dcounter, g.wcount, g.work, cap));
    CHK(LAUNCH(e, k_topk_pairs_bygroup<K>, dim3(8192), dim3(64), 0, cb->v, ds->d_rows, ds->n, first, tie_knn, g.gcnt, g.glist, cap_g, dcounter,
        g.wcount, g.work, cap, dpart));
  }
  else
    CHK(LAUNCH(e, k_topk_pairs<K>, dim3(1024), dim3(256), 0, cb->v, ds->d_rows, ds->n, first, tie_knn, dpairs, dcounter, dpart));
  CHK(LAUNCH(e, k_topk_merge<K>, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, count, dspan, dpart, dcounter, d_keys,
      e->d_stats + STAT_TOPK_PAIRS));
  // list full (dcounter[1] != 0, seen on the device: no host round trip): every sample through the one-wave kernel
  return LAUNCH(e, k_rerank_topk<K>, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, cb->v, ds->d_rows, ds->n, first, count, p.bpad, b.wmin, b.tau,
                tie_knn, d_keys, dcounter + 1);
}

// f(integral_constant<int, K>) for the top-K width K (1, 2, 4, 8) holding knn (1..8) neighbours; who: knn must be K
template <class F>
static int with_topk_width(int knn, const char *who, F f) {
  const int k = knn == 1 ? 1 : knn == 2 ? 2 : knn <= 4 ? 4 : 8;
  if (who && k != knn) return fail("%s: knn must be 1, 2, 4 or 8", who);
  if (k == 1) return f(std::integral_constant<int, 1>());
  if (k == 2) return f(std::integral_constant<int, 2>());
  return k == 4 ? f(std::integral_constant<int, 4>()) : f(std::integral_constant<int, 8>());
}
// f(integral_constant<int, v>) for the runtime value v, which must be one of Vs (else an error, not a launch): the SOM
// update's launches (host_som.inc) turn their plan's choices into template arguments with it; f returns 0 or an error
template <int V, int... Vs, class F>
static int with_value(int v, F &&f) {
  if (v == V) return f(std::integral_constant<int, V>());
  if constexpr (sizeof...(Vs) > 0) return with_value<Vs...>(v, f);
  else return fail("with_value: no launch built for the value %d", v);
}

extern "C" int somhip_debug_prefilter(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                                      float *wmin, float *tau, int64_t *bpad) try {
  CHK(check_pair(cb, ds, "somhip_debug_prefilter"));
  somhip_engine *e = cb->e;
  const ScanPlan p = scan_plan(cb, ds, count, 0);
  if (p.route != ROUTE_ONE_LEVEL) return fail("somhip_debug_prefilter: no pre-filter in this mode");
  HIPCHK(hipSetDevice(e->device));
  PrefilterBufs b;
  CHK(pf_filter(cb, ds, first, count, p, &b, nullptr, false, false));
  CHK(to_host(e, wmin, b.wmin, (size_t)cb->v.ngroups * p.bpad));
  CHK(to_host_sync(e, tau, b.tau, (size_t)count));
  if (bpad) *bpad = p.bpad;
  return 0;
} ABI_CATCH(somhip_debug_prefilter)
// prepare + level 1 alone, by the kernel the caller names: the ring kernel and the wide-tile kernel behind k_group_min
// are two witnesses of the same group minima
extern "C" int somhip_debug_level1(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int ring,
                                   float *wmin, uint32_t *gmin1, int64_t *bpad) try {
  CHK(check_pair(cb, ds, "somhip_debug_level1"));
  if (!wmin || !gmin1) return fail("somhip_debug_level1: null output");
  if (count <= 0 || first < 0 || first + count > ds->n) return fail("somhip_debug_level1: rows [%lld, +%lld) of %lld", (long long)first, (long long)count, (long long)ds->n);
  somhip_engine *e = cb->e;
  ScanPlan p = scan_plan(cb, ds, count, 1);
  if (!p.bf16 || p.route == ROUTE_MASKED) return fail("somhip_debug_level1: no bf16 level 1 in this mode");
  if ((p.d8 % 8) != 0 || p.nsb < 8 || p.bpad > 65535)
    return fail("somhip_debug_level1: %d k-steps, %lld sample tiles: neither level-1 kernel takes this shape", p.d8, (long long)p.nsb);
  p.route = ROUTE_TWO_LEVEL;
  p.kth = 1;
  p.l1_ring = ring != 0;
  p.l1_wide = true;
  HIPCHK(hipSetDevice(e->device));
  e->xc_phase = XC_NONE;
  PrefilterBufs b;
  CHK(bind_prefilter(cb, p, false, &b));
  CHK(pf_prepare(cb, ds, first, count, p, b, nullptr, false));
  CHK(pf_level1(cb, count, p, b, nullptr));
  CHK(to_host(e, wmin, b.wmin, (size_t)cb->v.ngroups * p.bpad));
  CHK(to_host_sync(e, gmin1, b.gmin1, (size_t)p.bpad));
  if (bpad) *bpad = p.bpad;
  return 0;
} ABI_CATCH(somhip_debug_level1)
// what pf_prepare leaves behind for a nearest-row search of these rows, on the bf16 pre-filter routes
extern "C" int somhip_debug_prepared(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                                     uint16_t *chi, uint16_t *clo, float *cn, float *rowmajor, uint16_t *xhi, uint16_t *xlo,
                                     uint16_t *xrow, float *tau, float *tau1, int32_t *info) try {
  CHK(check_pair(cb, ds, "somhip_debug_prepared"));
  if (!info) return fail("somhip_debug_prepared: null output");
  if (count <= 0 || first < 0 || first >= ds->n) return fail("somhip_debug_prepared: rows [%lld, +%lld) of %lld", (long long)first, (long long)count, (long long)ds->n);   // (the window may wrap)
  somhip_engine *e = cb->e;
  const ScanPlan p = scan_plan(cb, ds, count, 1);
  if (!p.bf16 || (p.route != ROUTE_ONE_LEVEL && p.route != ROUTE_TWO_LEVEL)) return fail("somhip_debug_prepared: no bf16 pre-filter for this search");
  HIPCHK(hipSetDevice(e->device));
  e->xc_phase = XC_NONE;
  const bool two = p.route == ROUTE_TWO_LEVEL;
  PrefilterBufs b;
  CHK(bind_prefilter(cb, p, false, &b));
  cb->prep_valid = cb->rowmajor_valid = false;           // the codebook pass itself is what the caller asks about
  CHK(pf_prepare(cb, ds, first, count, p, b, nullptr, false));
  const size_t ctile = sizeof(uint4) * (size_t)cb->v.ngroups * p.d8 * WAVE, xtile = sizeof(uint4) * (size_t)p.nsb * p.d8 * 32;
  const bool has_lo = !two || p.l2_global;
  auto get = [&](void *dst, const void *src, size_t bytes) { return dst && src ? to_host(e, (uint8_t *)dst, (const uint8_t *)src, bytes) : 0; };
  CHK(get(chi, cb->d_chi, ctile));
  CHK(get(clo, cb->d_clo, ctile));
  CHK(get(cn, cb->d_cn, sizeof(float) * (size_t)cb->v.ngroups * WAVE));
  CHK(get(rowmajor, cb->rowmajor_valid ? cb->d_rowmajor : nullptr, sizeof(float) * (size_t)cb->v.ngroups * WAVE * cb->v.d));
  CHK(get(xhi, b.xhi, xtile));
  CHK(get(xlo, has_lo ? b.xlo : nullptr, xtile));
  CHK(get(xrow, two ? b.xrow : nullptr, 2 * xtile));
  CHK(get(tau, b.tau, sizeof(float) * (size_t)count));
  CHK(get(tau1, two ? b.tau1 : nullptr, sizeof(float) * (size_t)count));
  HIPCHK(hipStreamSynchronize(e->stream));
  info[0] = cb->rowmajor_valid; info[1] = has_lo; info[2] = two; info[3] = p.d8;
  return 0;
} ABI_CATCH(somhip_debug_prepared)
// the cache of prepared copies as it lies on the device, and its flags: nothing is launched, no flag changes
extern "C" int somhip_debug_prepared_state(somhip_codebook *cb, int32_t *flags, uint16_t *chi, uint16_t *clo, float *cn,
                                           float *rowmajor) try {
  CHK(check_codebook(cb, flags != nullptr, "somhip_debug_prepared_state"));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const size_t slots = (size_t)cb->v.ngroups * WAVE, ctile = sizeof(uint4) * slots * (size_t)((cb->v.d4 + 1) / 2);
  auto get = [&](void *dst, const void *src, size_t bytes) { return dst && src ? to_host(e, (uint8_t *)dst, (const uint8_t *)src, bytes) : 0; };
  CHK(get(chi, cb->d_chi, ctile));
  CHK(get(clo, cb->d_clo, ctile));
  CHK(get(cn, cb->d_cn, sizeof(float) * slots));
  CHK(get(rowmajor, cb->d_rowmajor, sizeof(float) * slots * cb->v.d));
  HIPCHK(hipStreamSynchronize(e->stream));
  flags[0] = cb->prep_valid; flags[1] = cb->rowmajor_valid; flags[2] = cb->bm_open; flags[3] = cb->bm_moved;
  return 0;
} ABI_CATCH(somhip_debug_prepared_state)
// the nearest-row search of these rows with the selection of the re-rank's pairs by the kernel the caller names
extern "C" int somhip_debug_rerank_pairs(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int from_lists,
                                         float *wmin, uint64_t *wmask, uint32_t *gmin, float *tau, uint32_t *colcount,
                                         uint32_t *overflow, uint32_t *pairs, int64_t pairs_cap, int64_t *npairs,
                                         uint64_t *keys, int64_t *bpad) try {
  CHK(check_pair(cb, ds, "somhip_debug_rerank_pairs"));
  if (!wmin || !wmask || !gmin || !tau || !colcount || !overflow || !pairs || !npairs || !keys) return fail("somhip_debug_rerank_pairs: null output");
  if (count <= 0 || first < 0 || first >= ds->n) return fail("somhip_debug_rerank_pairs: rows [%lld, +%lld) of %lld", (long long)first, (long long)count, (long long)ds->n);   // (the window may wrap)
  somhip_engine *e = cb->e;
  const ScanPlan p = scan_plan(cb, ds, count, 1);
  if (p.route != ROUTE_ONE_LEVEL && p.route != ROUTE_TWO_LEVEL) return fail("somhip_debug_rerank_pairs: no pre-filter for this search");
  if (from_lists && p.route != ROUTE_TWO_LEVEL) return fail("somhip_debug_rerank_pairs: no level-2 lists on the one-level route");
  HIPCHK(hipSetDevice(e->device));
  uint64_t *dk;
  CHK(scratch(e, SLOT_CALL_A, (size_t)count, &dk));
  e->samples_searched += (uint64_t)count;
  PrefilterBufs b;
  CHK(pf_filter(cb, ds, first, count, p, &b, dk, false, p.fused_gmin));
  CHK(pf_rerank(cb, ds, first, count, p, b, dk, p.fused_gmin, nullptr, from_lists != 0));
  const size_t cells = (size_t)cb->v.ngroups * p.bpad;
  RerankPairs pl;                                  // the list pf_rerank filled
  CHK(bind_rerank_pairs(e, p.bpad, &pl));
  CHK(to_host(e, wmin, b.wmin, cells));
  CHK(to_host(e, wmask, b.wmask, cells));
  CHK(to_host(e, gmin, b.gmin, (size_t)p.bpad));
  CHK(to_host(e, tau, b.tau, (size_t)count));
  CHK(to_host(e, colcount, b.colcount, 4 * (size_t)pl.ncols));
  CHK(to_host(e, overflow, b.paircount, 1));
  CHK(to_host_sync(e, keys, dk, (size_t)count));
  // the segments' filled parts, one after another
  int64_t total = 0;
  for (uint32_t c = 0; c < pl.ncols; c++) {
    const int64_t n = std::min<uint32_t>(colcount[c], pl.cap_col);
    if (total + n > pairs_cap) return fail("somhip_debug_rerank_pairs: %lld pairs and more, room for %lld", (long long)(total + n), (long long)pairs_cap);
    if (n) CHK(to_host(e, pairs + 2 * total, reinterpret_cast<const uint32_t *>(pl.pairs + (size_t)c * pl.cap_col), 2 * (size_t)n));
    total += n;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  *npairs = total;
  if (bpad) *bpad = p.bpad;
  return 0;
} ABI_CATCH(somhip_debug_rerank_pairs)
extern "C" int somhip_debug_scan_plan(somhip_codebook *cb, somhip_dataset *ds, int64_t count, int want, int32_t *out) try {
  CHK(check_pair(cb, ds, "somhip_debug_scan_plan"));
  if (!out) return fail("somhip_debug_scan_plan: null output");
  const bool wide = want > 8 && want <= SOMHIP_KNN_MAX;
  if (want != 1 && want != 2 && want != 4 && want != 8 && !wide)
    return fail("somhip_debug_scan_plan: want %d is not 1, 2, 4, 8 or 9 .. %d", want, SOMHIP_KNN_MAX);
  if (count <= 0) return fail("somhip_debug_scan_plan: count %lld < 1", (long long)count);
  const ScanPlan p = scan_plan(cb, ds, count, want);
  out[0] = (int32_t)p.route; out[1] = p.kth; out[2] = p.bf16; out[3] = p.l1_ring;
  out[4] = p.by_group; out[5] = p.l2_global; out[6] = p.fused_gmin; out[7] = 0;
  if (wide) out[1] = (int32_t)p.chunk;
  return 0;
} ABI_CATCH(somhip_debug_scan_plan)
extern "C" int somhip_batch_winner_keys(somhip_codebook *cb, somhip_dataset *ds, int64_t first,
                                        int64_t count, uint64_t *dev_keys) try {
  CHK(check_pair(cb, ds, "somhip_batch_winner_keys"));
  if (count <= 0) return 0;
  HIPCHK(hipSetDevice(cb->e->device));
  bool nonneg = false;
  CHK(scan_keys_top1(cb, ds, first, count, dev_keys, &nonneg));
  if (!nonneg)
    CHK(LAUNCH(cb->e, k_clamp_keys, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, dev_keys, count));
  return 0;
} ABI_CATCH(somhip_batch_winner_keys)

// X1 with the pre-filter's bounds exchanged between the shards (kernels.hpp K2x): begin -> MIN all-reduce of the
// bounds -> refine -> MIN all-reduce -> finish -> MIN all-reduce of the keys.  Same keys as somhip_batch_winner_keys
// after the last all-reduce; every shard re-ranks only what the WHOLE codebook's search would.
extern "C" int somhip_shard_exchange_available(somhip_codebook *cb, somhip_dataset *ds, int64_t count) try {
  if (check_pair(cb, ds, "somhip_shard_exchange_available")) return 0;
  return scan_plan(cb, ds, count, 1).route == ROUTE_TWO_LEVEL && !getenv("SOMHIP_NO_SHARD_EXCHANGE") ? 1 : 0;
} catch (...) { return 0; }
// One call of an exchanged search: the checks, then run(plan, buffers).  The calls of ONE search run in order on the
// same codebook / data / range, handing their state over in scratch; `after`: the e->xc_phase this call continues.
template <class Run>
static int shard_call(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, XcState after, bool bufs_ok,
                      const char *who, Run run) {
  CHK(check_pair(cb, ds, who));
  if (count <= 0) return 0;
  if (!bufs_ok) return fail("%s: null buffer", who);
  if (!somhip_shard_exchange_available(cb, ds, count)) return fail("%s: not available for this shape (ask somhip_shard_exchange_available; use somhip_batch_winner_keys)", who);
  HIPCHK(hipSetDevice(cb->e->device));
  somhip_engine *e = cb->e;
  const bool continues = after == XC_NONE || (e->xc_phase == after && e->xc_cb == cb && e->xc_ds == ds && e->xc_first == first && e->xc_count == count);
  const int was = e->xc_phase;
  e->xc_phase = XC_NONE;                           // (until this call has run)
  if (!continues) return fail("%s: not the continuation of the search somhip_shard_winner_begin started on this engine (phase %d after %d)", who, after + 1, was);
  if (after == XC_NONE) e->samples_searched += (uint64_t)count;
  const ScanPlan p = scan_plan(cb, ds, count, 1);
  PrefilterBufs b;
  CHK(bind_prefilter(cb, p, true, &b));
  CHK(run(p, b));
  e->xc_phase = after == XC_REFINED ? XC_NONE : after + 1; e->xc_cb = cb; e->xc_ds = ds; e->xc_first = first; e->xc_count = count;
  return 0;
}
extern "C" int somhip_shard_winner_begin(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                                         uint64_t *dev_keys, float *dev_bound) try {
  return shard_call(cb, ds, first, count, XC_NONE, dev_bound && dev_keys, "somhip_shard_winner_begin", [&](const ScanPlan &p, const PrefilterBufs &b) {
    CHK(pf_prepare(cb, ds, first, count, p, b, dev_keys, true));
    return pf_level1(cb, count, p, b, dev_bound);
  });
} ABI_CATCH(somhip_shard_winner_begin)
extern "C" int somhip_shard_winner_refine(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                                          float *dev_bound) try {
  return shard_call(cb, ds, first, count, XC_BEGUN, dev_bound, "somhip_shard_winner_refine", [&](const ScanPlan &p, const PrefilterBufs &b) {
    return pf_level2(cb, count, p, b, !getenv("SOMHIP_NO_FUSED_GMIN"), dev_bound);
  });
} ABI_CATCH(somhip_shard_winner_refine)
extern "C" int somhip_shard_winner_finish(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                                          const float *dev_bound, uint64_t *dev_keys) try {
  return shard_call(cb, ds, first, count, XC_REFINED, dev_bound && dev_keys, "somhip_shard_winner_finish", [&](const ScanPlan &p, const PrefilterBufs &b) {
    return pf_rerank(cb, ds, first, count, p, b, dev_keys, true, dev_bound, true);      // (refine formed the group minima; an exchange is two-level)
  });
} ABI_CATCH(somhip_shard_winner_finish)

// X2 (SURVEY 8e): this shard's k best rows per sample as packed keys, ascending; a host all-gathers
// the shards' lists and keeps the k smallest per sample (keys are unique: tag = global row, or its
// complement for the k-NN tie order, so the merge IS find_winner_knn over the whole codebook).
// Masked data sets: K1m (knn 1) / K1mk (knn 2, 4, 8); fully masked samples are the caller's to skip.
extern "C" int somhip_batch_topk_keys(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count,
                                      int knn, int tie, uint64_t *dev_keys) try {
  CHK(check_pair(cb, ds, "somhip_batch_topk_keys"));
  if (knn < 1 || knn > 8) return fail("somhip_batch_topk_keys: knn %d not in 1..8", knn);
  if (count <= 0) return 0;
  HIPCHK(hipSetDevice(cb->e->device));
  const int t = tie == SOMHIP_TIE_KNN ? 1 : 0;
  if (knn == 1 && t) return fail("somhip_batch_topk_keys: knn 1 is find_winner_euc (SOMHIP_TIE_FIRST)");
  return with_topk_width(knn, "somhip_batch_topk_keys", [&](auto k) {
    if constexpr (decltype(k)::value == 1) return somhip_batch_winner_keys(cb, ds, first, count, dev_keys);
    else return scan_keys_topk<decltype(k)::value>(cb, ds, first, count, dev_keys, t);
  });
} ABI_CATCH(somhip_batch_topk_keys)

static void decode_key(uint64_t k, bool inverted, int32_t *index, float *diff) {
  uint32_t bits = (uint32_t)(k >> 32);
  uint32_t tag = (uint32_t)k;
  if (bits >= FLT_MAX_BITS) { *index = -1; *diff = -1.0f; return; }   // nothing beat FLT_MAX (lvq_pak.c:56)
  *index = (int32_t)(inverted ? ~tag : tag);
  memcpy(diff, &bits, 4);
}

// the outputs of one sample of somhip_find_winners from its knn keys (empty: every component masked)
static void decode_sample(const uint64_t *k, int knn, bool knn_rule, bool empty, int32_t *index, float *diff, int32_t *ret) {
  for (int j = 0; j < knn; j++) {
    if (empty) { index[j] = -2; diff[j] = -1.0f; }
    else decode_key(k[j], knn_rule, index + j, diff + j);
  }
  if (ret) *ret = empty ? 0 : knn;
}

extern "C" int somhip_knn_max(void) { return SOMHIP_KNN_MAX; }
static_assert(SOMHIP_KNN_MAX == KNN_WIDE_MAX, "the select stage's pool is laid out for SOMHIP_KNN_MAX neighbours");

// The device keys of a k-NN search over a run of samples, chunk by chunk: what somhip_find_winners and somhip_knn_vote
// share.  knn 1: the nearest row (scan_keys_top1, plain tags); 2 .. 8: the top-K routes with K = 2, 4 or 8 keys per sample
// (with_topk_width), chunks of 4096; 9 .. SOMHIP_KNN_MAX: the wide route (K1w), masked data or not -- pack the samples,
// every distance, the select -- in chunks of ScanPlan::chunk.  use(off, f, c, dk, stride) runs per chunk behind the
// launches that leave keys dk[c][stride] (ascending, the first knn count) in SLOT_CALL_A for the c samples from data
// row f on, the run's samples off .. off + c - 1; it returns 0 or an error.  tie_knn: the order of equal distances for
// knn 2 .. 8 -- 1: find_winner_knn's, tags ~unit; 0: SOMHIP_TIE_FIRST, plain tags (somhip_map_quality).  The wide route
// has find_winner_knn's order only.
template <class Use>
static int knn_chunk_keys(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int knn, int tie_knn, Use use) {
  somhip_engine *e = cb->e;
  if (knn <= 8)
    return with_topk_width(knn, nullptr, [&](auto width) {
      constexpr int KK = decltype(width)::value;
      const int64_t CH = std::min<int64_t>(4096, count);
      uint64_t *dk;
      CHK(scratch(e, SLOT_CALL_A, (size_t)CH * KK, &dk));
      for (int64_t off = 0; off < count; off += CH) {
        const int64_t c = std::min(CH, count - off);
        const int64_t f = (first + off) % ds->n;
        if constexpr (KK == 1) CHK(scan_keys_top1(cb, ds, f, c, dk));
        else CHK(scan_keys_topk<KK>(cb, ds, f, c, dk, tie_knn));
        CHK(use(off, f, c, dk, KK));
      }
      return 0;
    });
  const ScanPlan p = scan_plan(cb, ds, count, knn);
  const int64_t CH = std::min(p.chunk, count), ld = cb->v.ngroups * WAVE;
  const unsigned nblk = (unsigned)((cb->v.ngroups + 3) / 4);
  float *dist; uint64_t *dk;
  CHK(scratch(e, SLOT_KNN_DIST, (size_t)CH * ld, &dist));
  CHK(scratch(e, SLOT_CALL_A, (size_t)CH * knn, &dk));
  for (int64_t off = 0; off < count; off += CH) {
    const int64_t c = std::min(CH, count - off);
    const int64_t f = (first + off) % ds->n;
    if (ds->d_mask) {
      CHK(LAUNCH_TIMED(e, KID_KNN_DIST, k_knn_dist_masked, dim3(nblk, (unsigned)c), dim3(256), 0, cb->v, ds->d_rows, ds->d_mask, ds->n, f, ld, dist));
    } else {
      const int64_t nsb = (c + SCAN_S - 1) / SCAN_S;
      float4 *xt;
      CHK(scratch(e, SLOT_SAMPLES, (size_t)nsb * cb->v.d4 * SCAN_S, &xt));
      CHK(LAUNCH_TIMED(e, KID_PACK_SAMPLES, k_pack_samples<SCAN_S>, dim3((unsigned)nsb), dim3(256), 0, ds->d_rows, ds->n, ds->d, cb->v.d4, f, c, xt));
      CHK(LAUNCH_TIMED(e, KID_KNN_DIST, k_knn_dist<SCAN_S>, dim3((unsigned)nsb, nblk), dim3(256), 0, cb->v, xt, c, ld, dist));
      e->samples_searched += (uint64_t)c;
    }
    CHK(LAUNCH_TIMED(e, KID_KNN_SELECT, k_knn_select, dim3((unsigned)c), dim3(KNN_THREADS), 0, cb->v, dist, ld, knn, dk));
    CHK(use(off, f, c, dk, knn));
  }
  return 0;
}
// HIP-event totals of the wide route's two stages since somhip_timing_reset, while somhip_timing_enable is on (timed under
// ids of their own, like the map-set kernels): [0] the distance stage (k_knn_dist / k_knn_dist_masked), [1] k_knn_select
extern "C" int somhip_knn_timing(somhip_engine *e, int64_t launches[2], double total_ms[2]) try {
  const int kid[2] = {KID_KNN_DIST, KID_KNN_SELECT};
  return stage_timing(e, "somhip_knn_timing", kid, 2, launches, total_ms);
} ABI_CATCH(somhip_knn_timing)

// find_winner_euc / find_winner_knn over a run of samples (include/somhip.h); masked data sets take K1m / K1mk for
// knn <= 8, and a fully masked sample reports ret 0, index -2 (lvq_pak.c:65-69 / :188-189 return 0 neighbours);
// knn 9 .. SOMHIP_KNN_MAX: the wide route.  Per chunk (knn_chunk_keys): the keys, one copy of them, decode
extern "C" int somhip_find_winners(somhip_codebook *cb, somhip_dataset *ds, int64_t first,
                                   int64_t count, int knn, int tie, int32_t *index, float *diff,
                                   int32_t *ret) try {
  CHK(check_pair(cb, ds, "somhip_find_winners"));
  if (knn < 1 || knn > SOMHIP_KNN_MAX) return fail("somhip_find_winners: knn %d not in 1..%d", knn, SOMHIP_KNN_MAX);
  if (!index || !diff) return fail("somhip_find_winners: null output");
  if (count <= 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  // find_winner_knn(knn == 1) IS find_winner_euc (lvq_pak.c:160-161)
  const bool knn_rule = (tie == SOMHIP_TIE_KNN) && knn >= 2;
  if (!knn_rule && knn != 1) return fail("somhip_find_winners: knn > 1 needs SOMHIP_TIE_KNN");
  std::vector<uint64_t> hk;
  return knn_chunk_keys(cb, ds, first, count, knn, 1, [&](int64_t off, int64_t f, int64_t c, const uint64_t *dk, int stride) {
    if (hk.empty()) hk.resize((size_t)c * stride);                      // (the first chunk is the longest)
    CHK(to_host_sync(e, hk.data(), dk, (size_t)c * stride));
    for (int64_t i = 0; i < c; i++) {
      const bool empty = sample_is_empty(ds, (f + i) % ds->n);
      decode_sample(hk.data() + (size_t)i * stride, knn, knn_rule, empty, index + (off + i) * knn, diff + (off + i) * knn,
                    ret ? ret + off + i : nullptr);
    }
    return 0;
  });
} ABI_CATCH(somhip_find_winners)

// the device copy of a data set's row labels, made when first wanted (none for a data set without labels)
static int dataset_device_labels(somhip_dataset *ds) {
  if (ds->labels.empty() || ds->d_labels) return 0;
  HIPCHK(hipMalloc((void **)&ds->d_labels, sizeof(int32_t) * (size_t)ds->n));
  HIPCHK(hipMemcpy(ds->d_labels, ds->labels.data(), sizeof(int32_t) * (size_t)ds->n, hipMemcpyHostToDevice));
  return 0;
}

// K1v: the class vote of find_winner_knn's neighbours over a run of samples (include/somhip.h).  Per chunk
// (knn_chunk_keys, so the routes, the chunks, the wrap and masked data are somhip_find_winners'): the keys, k_knn_vote
// behind them, one copy of 16 bytes per sample.  A sample with every component masked has no neighbours, whatever its keys say.
extern "C" int somhip_knn_vote(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, int knn,
                               int32_t *label, int32_t *freq, int32_t *own, int32_t *found) try {
  CHK(check_pair(cb, ds, "somhip_knn_vote"));
  if (knn < 1 || knn > SOMHIP_KNN_MAX) return fail("somhip_knn_vote: knn %d not in 1..%d", knn, SOMHIP_KNN_MAX);
  if (!label) return fail("somhip_knn_vote: null output");
  if (!cb->d_labels) return fail("somhip_knn_vote: codebook has no labels");
  if (is_shard(cb))
    return fail("somhip_knn_vote: sharded codebook not supported (a shard does not hold the other shards' labels)");
  if (first < 0) return fail("somhip_knn_vote: first row %lld < 0", (long long)first);
  if (count <= 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  CHK(dataset_device_labels(ds));
  std::vector<int32_t> hv;
  return knn_chunk_keys(cb, ds, first, count, knn, 1, [&](int64_t off, int64_t f, int64_t c, const uint64_t *dk, int stride) {
    int4 *dv;
    CHK(scratch(e, SLOT_CALL_B, (size_t)c, &dv));
    CHK(LAUNCH_TIMED(e, KID_KNN_VOTE, k_knn_vote, dim3((unsigned)((c + VOTE_SAMPLES - 1) / VOTE_SAMPLES)), dim3(VOTE_SAMPLES * WAVE), 0, dk, stride,
        knn, knn >= 2 ? 1 : 0, cb->d_labels, cb->v.row_offset, cb->v.n, ds->d_labels, f, ds->n, c, dv));
    if (hv.empty()) hv.resize(4 * (size_t)c);                           // (the first chunk is the longest)
    CHK(to_host_sync(e, hv.data(), reinterpret_cast<const int32_t *>(dv), 4 * (size_t)c));
    for (int64_t i = 0; i < c; i++) {
      const int32_t *v = hv.data() + 4 * (size_t)i;
      const bool empty = sample_is_empty(ds, (f + i) % ds->n);
      label[off + i] = empty ? -1 : v[0];
      if (freq) freq[off + i] = empty ? 0 : v[1];
      if (own) own[off + i] = ds->d_labels ? (empty ? 0 : v[2]) : -1;
      if (found) found[off + i] = empty ? 0 : v[3];
    }
    return 0;
  });
} ABI_CATCH(somhip_knn_vote)
// HIP-event total of k_knn_vote since somhip_timing_reset, while somhip_timing_enable is on (an id of its own behind the
// published table, like the wide route's stages)
extern "C" int somhip_knn_vote_timing(somhip_engine *e, int64_t *launches, double *total_ms) try {
  const int kid[1] = {KID_KNN_VOTE};
  return stage_timing(e, "somhip_knn_vote_timing", kid, 1, launches, total_ms);
} ABI_CATCH(somhip_knn_vote_timing)

// lininit's data passes (find_eigenvectors, som_rout.c:211-289): per-component sums / counts over the
// unmasked entries, then the upper triangle (j >= i) of sum_r (x_ri - mean_i)(x_rj - mean_j); every
// element accumulated over the rows in file order, in fp32, like the reference.
extern "C" int somhip_column_sums(somhip_dataset *ds, float *sum, int64_t *count) try {
  CHK(check_dataset(ds, sum && count, "somhip_column_sums"));
  somhip_engine *e = ds->e;
  HIPCHK(hipSetDevice(e->device));
  float *dsum; unsigned long long *dcnt;
  CHK(scratch(e, SLOT_CALL_A, (size_t)ds->d, &dsum));
  CHK(scratch(e, SLOT_CALL_B, (size_t)ds->d, &dcnt));
  CHK(LAUNCH(e, k_column_sums, dim3((unsigned)((ds->d + 255) / 256)), dim3(256), 0, ds->d_rows, ds->d_mask, ds->n, ds->d, dsum, dcnt));
  std::vector<unsigned long long> hc((size_t)ds->d);
  CHK(to_host(e, sum, dsum, (size_t)ds->d));
  CHK(to_host_sync(e, hc.data(), dcnt, (size_t)ds->d));
  for (int i = 0; i < ds->d; i++) count[i] = (int64_t)hc[(size_t)i];
  return 0;
} ABI_CATCH(somhip_column_sums)

extern "C" int somhip_centered_products(somhip_dataset *ds, const float *mean, float *r) try {
  CHK(check_dataset(ds, mean && r, "somhip_centered_products"));
  somhip_engine *e = ds->e;
  HIPCHK(hipSetDevice(e->device));
  const size_t dd = (size_t)ds->d * ds->d;
  float *dmean, *dr;
  CHK(scratch(e, SLOT_CALL_A, (size_t)ds->d, &dmean));
  CHK(scratch(e, SLOT_CALL_B, dd, &dr));
  CHK(to_device(e, dmean, mean, (size_t)ds->d));
  HIPCHK(hipMemsetAsync(dr, 0, sizeof(float) * dd, e->stream));
  const unsigned nb = (unsigned)((ds->d + 15) / 16);
  CHK(LAUNCH(e, k_centered_products, dim3(nb, nb), dim3(256), 0, ds->d_rows, ds->d_mask, ds->n, ds->d, dmean, dr));
  CHK(to_host_sync(e, r, dr, dd));
  return 0;
} ABI_CATCH(somhip_centered_products)

// randinit's data pass (randinit_codes, som_rout.c:98-131): smallest / largest unmasked value and their number
// per component.  The reference's seeds (FLT_MIN for the maximum, FLT_MAX for the minimum, :108-111) are the
// caller's business; components without data come back as lo = +FLT_MAX, hi = -FLT_MAX, count 0.
extern "C" int somhip_column_minmax(somhip_dataset *ds, float *lo, float *hi, int64_t *count) try {
  CHK(check_dataset(ds, lo && hi, "somhip_column_minmax"));
  somhip_engine *e = ds->e;
  HIPCHK(hipSetDevice(e->device));
  uint32_t *dmin; unsigned long long *dcnt;
  CHK(scratch(e, SLOT_CALL_A, 2 * (size_t)ds->d, &dmin));      // the minima, then the maxima
  CHK(scratch(e, SLOT_CALL_B, (size_t)ds->d, &dcnt));
  uint32_t *dmax = dmin + ds->d;
  HIPCHK(hipMemsetAsync(dmin, 0xFF, sizeof(uint32_t) * (size_t)ds->d, e->stream));
  HIPCHK(hipMemsetAsync(dmax, 0, sizeof(uint32_t) * (size_t)ds->d, e->stream));
  HIPCHK(hipMemsetAsync(dcnt, 0, sizeof(unsigned long long) * (size_t)ds->d, e->stream));
  const int64_t nblk = std::max<int64_t>(1, std::min<int64_t>(2048, (ds->n + 255) / 256));
  const int64_t per = (ds->n + nblk - 1) / nblk;
  CHK(LAUNCH(e, k_column_minmax, dim3((unsigned)((ds->d + 255) / 256), (unsigned)((ds->n + per - 1) / per)), dim3(256), 0, ds->d_rows, ds->d_mask,
      ds->n, ds->d, per, dmin, dmax, dcnt));
  std::vector<uint32_t> hm(2 * (size_t)ds->d);
  std::vector<unsigned long long> hc((size_t)ds->d);
  CHK(to_host(e, hm.data(), dmin, 2 * (size_t)ds->d));
  CHK(to_host_sync(e, hc.data(), dcnt, (size_t)ds->d));
  auto back = [](uint32_t o) { uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; float f; memcpy(&f, &b, 4); return f; };
  for (int i = 0; i < ds->d; i++) {
    if (hc[(size_t)i]) { lo[i] = back(hm[(size_t)i]); hi[i] = back(hm[(size_t)ds->d + i]); }
    else { lo[i] = 3.402823466e+38f; hi[i] = -3.402823466e+38f; }
    if (count) count[i] = (int64_t)hc[(size_t)i];
  }
  return 0;
} ABI_CATCH(somhip_column_minmax)

// find_qerror2 (som_rout.c:823-885): out[i] = the neighbourhood-weighted error of sample first+i
// (0 where the sample has no winner); the caller adds them in data order, as the reference does.
extern "C" int somhip_qerror2(somhip_codebook *cb, somhip_dataset *ds, float radius, int64_t first,
                              int64_t count, float *out, int32_t *ret) try {
  CHK(check_pair(cb, ds, "somhip_qerror2"));
  if (!out) return fail("somhip_qerror2: null output");
  if (cb->v.topol != SOMHIP_TOPOL_HEXA && cb->v.topol != SOMHIP_TOPOL_RECT) return fail("somhip_qerror2: can't set SOM parameters");
  if (is_shard(cb)) return fail("somhip_qerror2: sharded codebook not supported");
  if (count <= 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const bool gauss = cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN;
  const float thresh = gauss ? 0.0f : bubble_threshold(radius);
  double reach = radius > 0.0f ? (double)radius / (cb->v.topol == SOMHIP_TOPOL_RECT ? 1.0 : 0.8660254037844386) + 1.0 : 1.0;
  const int ireach = reach > 1e6 ? 1000000 : (int)reach;
  const int64_t CH = 4096;
  uint64_t *dk; float *dq;
  CHK(scratch(e, SLOT_CALL_A, (size_t)std::min(CH, count), &dk));
  CHK(scratch(e, SLOT_CALL_B, (size_t)std::min(CH, count), &dq));
  const size_t dyn = (size_t)cb->v.d * 5 + 16;
  for (int64_t off = 0; off < count; off += CH) {
    const int64_t c = std::min(CH, count - off);
    const int64_t f = (first + off) % ds->n;
    CHK(scan_keys_top1(cb, ds, f, c, dk));
    CHK(launch(e, "k_qerror2", gauss ? k_qerror2<true> : k_qerror2<false>, dim3((unsigned)c), dim3(256), dyn, cb->v, cb->ydim, ds->d_rows, ds->d_mask,
               ds->n, f, dk, radius, thresh, ireach, dq));
    CHK(to_host_sync(e, out + off, dq, (size_t)c));
    // a sample with every component masked has no winner, whatever its key says (every distance is an empty sum, 0):
    // the kernel's sum over zero distances is 0 too, except where the rate itself is NaN (gaussian, radius 0)
    for (int64_t i = 0; i < c; i++) {
      const bool empty = sample_is_empty(ds, (f + i) % ds->n);
      if (empty) out[off + i] = 0.0f;
      if (ret) ret[off + i] = empty ? 0 : 1;
    }
  }
  return 0;
} ABI_CATCH(somhip_qerror2)
