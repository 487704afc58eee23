// host_batchmap.inc -- K8, the batch map: per epoch the winners of every sample against the frozen codebook, the per-unit
// ordered fp64 sums (stage 1) and the neighbourhood combine on the fp64 MFMA (stage 2); the same epoch over data in pieces
// (somhip_batchmap_begin / _accumulate / _finish: the sums' chains continued from piece to piece) and over the row blocks
// of G ranks (somhip_som_batchmap_ranks)
// K8m, the same over data with missing values (somhip_som_batchmap_missing, somhip_batchmap_missing_*): the state holds a
// count per component, [S | C], the sums skip masked components and the combine divides per component.  Every entry
// point of either form is one body here, told which form it serves.
// (included by somhip.hip behind host_proto.inc: one translation unit, the trainers' shared checks)
#include <rocprim/device/device_radix_sort.hpp>

// The device arrays of a batch-map call.  SLOT_BATCHMAP, per unit: [S: units x (dim + 1) doubles][the gaussian table]
// [hits][starts: units + 1].  SLOT_BATCHMAP_LIST, per sample: [win][idx][the sorted winners][list][the sort's own room].
// The two forms of S, stated here once.  Plain: [S | hits], a unit's dim sums and behind them its one count.  Missing:
// [S | C] as units x 2 dim doubles, C following S per unit -- unit u's sums at [u * 2 dim, + dim), the counts of the same
// components at [u * 2 dim + dim, + dim).  A continued state is S in the same form, then the 16-byte tail.
struct BatchmapBufs {
  bool missing = false;               // the form of S
  double *S = nullptr, *table = nullptr;
  uint32_t *hits = nullptr, *starts = nullptr, *win = nullptr, *idx = nullptr, *win_sorted = nullptr, *list = nullptr;
  void *sort_tmp = nullptr;
  size_t sort_bytes = 0;
  unsigned sort_bits = 0;             // the winners' bits that differ: those of 0 .. units
};
static size_t batchmap_table_len(const somhip_codebook *cb) {
  return cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN ? 2 * (size_t)(2 * cb->v.xdim - 1) * (size_t)(2 * cb->ydim - 1) : 0;
}
// n: the samples of a sums stage, 0 where only the combine runs.  state (or null): S is the codebook's own continued
// accumulation, not engine scratch, and the slot holds the rest only.
static size_t batchmap_unit_doubles(const somhip_codebook *cb, bool missing) { return missing ? 2 * (size_t)cb->v.d : (size_t)cb->v.d + 1; }
static int batchmap_bind(somhip_codebook *cb, int64_t n, BatchmapBufs *b, double *state = nullptr, bool missing = false) {
  somhip_engine *e = cb->e;
  const size_t units = (size_t)cb->v.n, ns = (size_t)n, s_len = state ? 0 : units * batchmap_unit_doubles(cb, missing), t_len = batchmap_table_len(cb);
  void *p;
  b->missing = missing;
  CHK(engine_scratch(e, SLOT_BATCHMAP, sizeof(double) * (s_len + t_len) + sizeof(uint32_t) * (2 * units + 1), &p));
  b->S = state ? state : (double *)p;
  b->table = (double *)p + s_len;
  b->hits = reinterpret_cast<uint32_t *>(b->table + t_len);
  b->starts = b->hits + units;
  if (n <= 0) return 0;
  for (size_t u = units; u; u >>= 1) b->sort_bits++;
  const hipError_t er = rocprim::radix_sort_pairs(nullptr, b->sort_bytes, b->win, b->win_sorted, b->idx, b->list, ns, 0u, b->sort_bits, e->stream);
  if (er != hipSuccess) return fail("batch map: the sort's size query failed: %s", hipGetErrorString(er));
  const size_t arrays = (sizeof(uint32_t) * 4 * ns + 255) / 256 * 256;
  CHK(engine_scratch(e, SLOT_BATCHMAP_LIST, arrays + b->sort_bytes, &p));
  b->win = (uint32_t *)p;
  b->idx = b->win + ns;
  b->win_sorted = b->idx + ns;
  b->list = b->win_sorted + ns;
  b->sort_tmp = (char *)p + arrays;
  return 0;
}

// find_qerror's float chain over one sample's winner distance (d1 < 0: an empty vector, or one without a winner, as kept by
// batchmap_group_stage)
static inline void batchmap_q_step(float &q, float d1) { q += sqrt((double)d1); }   // float accumulator, som_rout.c:715

// Stage 1 (steps 2-3 of the definition, include/somhip.h), the group half: the winners of data rows (first + s) % n_rows,
// s < n, against the codebook as it stands, counted into b.hits and listed per unit in data order.  Per chunk
// (knn_chunk_keys with knn 1, SOMHIP_TIE_FIRST): the keys, k_batchmap_winners behind them; then the scan and the stable
// sort by winner.  q (or null: no per-sample copy leaves the device): find_qerror's float chain over the winners' distances
// in data order, as somhip_map_quality forms it, continued from *q.  keep (with q): the chain is not run; the distances
// it would take are kept in data order instead (-1 for a sample it skips), for a caller that learns where the chain
// starts only later.  kid: the timing id the stage's launches count under (map distortion runs it under its own).
static int batchmap_group_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const BatchmapBufs &b, float *q,
                                std::vector<float> *keep = nullptr, int kid = KID_BATCHMAP_GROUP) {
  somhip_engine *e = cb->e;
  const uint32_t units = (uint32_t)cb->v.n;
  HIPCHK(hipMemsetAsync(b.hits, 0, sizeof(uint32_t) * (size_t)units, e->stream));
  float chain = q ? *q : 0.0f;
  std::vector<float> hd;
  if (keep) keep->clear();
  CHK(knn_chunk_keys(cb, ds, first, n, 1, 0, [&](int64_t off, int64_t f, int64_t c, const uint64_t *dk, int stride) {
    float *dd1 = nullptr;
    if (q) CHK(scratch(e, SLOT_CALL_B, (size_t)c, &dd1));
    CHK(LAUNCH_TIMED(e, kid, k_batchmap_winners, dim3((unsigned)((c + BM_THREADS - 1) / BM_THREADS)), dim3(BM_THREADS), 0, dk,
        stride, off, c, units, b.win, b.idx, dd1, b.hits));
    if (!q) return 0;
    if (hd.empty()) hd.resize((size_t)c);                               // (the first chunk is the longest)
    CHK(to_host_sync(e, hd.data(), dd1, (size_t)c));
    for (int64_t i = 0; i < c; i++) {
      const bool skip = sample_is_empty(ds, (f + i) % ds->n);           // ignore empty vectors, som_rout.c:712
      if (keep) keep->push_back(skip ? -1.0f : hd[(size_t)i]);
      else if (!skip) batchmap_q_step(chain, hd[(size_t)i]);
    }
    return 0;
  }));
  CHK(LAUNCH_TIMED(e, kid, k_batchmap_starts, dim3(1), dim3(BM_SCAN_THREADS), 0, b.hits, units, b.starts));
  {
    LaunchTimer t(e, kid);                                              // (rocPRIM's own launches, on the engine's stream)
    size_t bytes = b.sort_bytes;
    const hipError_t er = rocprim::radix_sort_pairs(b.sort_tmp, bytes, b.win, b.win_sorted, b.idx, b.list, (size_t)n, 0u, b.sort_bits, e->stream);
    if (er != hipSuccess) return fail("batch map: the sort by winner failed: %s", hipGetErrorString(er));
  }
  if (q) *q = chain;
  return 0;
}
// ... and the sums half: b.S <- [S | hits], or [S | C] under the data's mask, from the lists.  cont: the chains and counts
// go on from what b.S holds.
static int batchmap_sums_launch(somhip_codebook *cb, somhip_dataset *ds, int64_t first, const BatchmapBufs &b, bool cont,
                                int kid = KID_BATCHMAP_SUMS) {
  somhip_engine *e = cb->e;
  if (b.missing) {
    const dim3 mgrid((unsigned)cb->v.n, (unsigned)((cb->v.d + BM_SUM_DIMS - 1) / BM_SUM_DIMS));
    if (cont)
      return LAUNCH_TIMED(e, kid, k_batchmap_sums_missing<true>, mgrid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->d_mask, ds->n, ds->d, first % ds->n,
                          b.list, b.starts, b.S);
    return LAUNCH_TIMED(e, kid, k_batchmap_sums_missing<false>, mgrid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->d_mask, ds->n, ds->d, first % ds->n,
                        b.list, b.starts, b.S);
  }
  const dim3 grid((unsigned)cb->v.n, (unsigned)((cb->v.d + 1 + BM_SUM_DIMS - 1) / BM_SUM_DIMS));
  if (cont)
    return LAUNCH_TIMED(e, kid, k_batchmap_sums<true>, grid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->n, ds->d, first % ds->n, b.list,
                        b.starts, b.S);
  return LAUNCH_TIMED(e, kid, k_batchmap_sums<false>, grid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->n, ds->d, first % ds->n, b.list,
                      b.starts, b.S);
}
static int batchmap_sums_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const BatchmapBufs &b, float *qerror) {
  if (qerror) *qerror = 0.0f;
  CHK(batchmap_group_stage(cb, ds, first, n, b, qerror));
  return batchmap_sums_launch(cb, ds, first, b, false);
}

// Stage 2 (steps 4-5): the codebook's rows <- (float)(N / D) from b.S at radius r, where D > 0, for the destination row
// groups [g0, g0 + groups) (groups < 0: all of them); rows of other groups keep their bits.
static int batchmap_combine_stage(somhip_codebook *cb, float r, const BatchmapBufs &b, int64_t g0 = 0, int64_t groups = -1) {
  somhip_engine *e = cb->e;
  const bool gauss = cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN;
  const int small_map = cb->v.xdim <= 1024 && cb->ydim <= 1024;         // (lattice_sq_small's condition)
  if (groups < 0) groups = cb->v.ngroups;
  if (groups == 0) return 0;
  const dim3 grid((unsigned)groups, (unsigned)((cb->v.d + BM_COLS - 1) / BM_COLS));
  const dim3 mgrid((unsigned)groups, (unsigned)((cb->v.d + BMM_COLS - 1) / BMM_COLS));
  rows_written(cb);                                                     // (the caller whose own state this is re-opens it)
  if (gauss) {
    const size_t t_len = batchmap_table_len(cb);
    CHK(LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_gauss_table, dim3((unsigned)((t_len + BM_THREADS - 1) / BM_THREADS)), dim3(BM_THREADS), 0,
        cb->v.topol, cb->v.xdim, cb->ydim, r, b.table));
    if (b.missing)
      return LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_combine_missing<true>, mgrid, dim3(256), 0, cb->v, cb->ydim, b.S, r, small_map, b.table, g0);
    return LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_combine<true>, grid, dim3(256), 0, cb->v, cb->ydim, b.S, r, small_map, b.table, g0);
  }
  if (b.missing)
    return LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_combine_missing<false>, mgrid, dim3(256), 0, cb->v, cb->ydim, b.S, bubble_threshold(r),
                        small_map, nullptr, g0);
  return LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_combine<false>, grid, dim3(256), 0, cb->v, cb->ydim, b.S, bubble_threshold(r), small_map,
                      nullptr, g0);
}

// what every batch-map entry point refuses before anything is launched
static int batchmap_check_codebook(const somhip_codebook *cb, const char *who) {
  if (is_shard(cb)) return fail("%s: sharded codebook not supported (a shard does not hold the other shards' units)", who);
  if ((cb->v.topol != SOMHIP_TOPOL_HEXA && cb->v.topol != SOMHIP_TOPOL_RECT) || (int64_t)cb->v.xdim * cb->ydim != cb->v.n)
    return fail("%s: codebook without a lattice (%d x %d units, %lld rows)", who, cb->v.xdim, cb->ydim, (long long)cb->v.n);
  if (cb->v.neigh != SOMHIP_NEIGH_BUBBLE && cb->v.neigh != SOMHIP_NEIGH_GAUSSIAN) return fail("%s: unknown neighbourhood %d", who, cb->v.neigh);
  return 0;
}
static int batchmap_check_data(const somhip_dataset *ds, int64_t first, int64_t n, const char *who, bool masks_ok = false) {
  if (ds->d_mask && !masks_ok) return fail("%s: data with masked components (x) is not supported", who);
  if (first < 0) return fail("%s: first row %lld < 0", who, (long long)first);
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  if (n >= (int64_t)1 << 32) return fail("%s: n %lld does not fit the 32-bit hit counts", who, (long long)n);
  return 0;
}

// The epochs of either form (missing: K8m, masks taken)
static int batchmap_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p, float *qerror_out, bool missing,
                          const char *who) {
  CHK(check_pair(cb, ds, who));
  if (!p) return fail("%s: null parameters", who);
  CHK(batchmap_check_codebook(cb, who));
  CHK(batchmap_check_data(ds, p->first, p->n, who, missing));
  CHK(check_epochs(p->epochs, who));
  if (!(p->radius >= 1.0f)) return fail("%s: radius %g < 1", who, (double)p->radius);
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  close_accumulations(cb);                                              // (the rows move: an open accumulation is over)
  BatchmapBufs b;
  CHK(batchmap_bind(cb, p->n, &b, nullptr, missing));
  for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
    const float r = 1.0f + linear_rate(p->radius - 1.0f, p->epochs, t);       // som_rout.c:615 over epochs
    CHK(batchmap_sums_stage(cb, ds, p->first, p->n, b, qerror_out ? qerror_out + (t - p->start_epoch) : nullptr));
    CHK(batchmap_combine_stage(cb, r, b));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}
extern "C" int somhip_som_batchmap(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p, float *qerror_out) try {
  return batchmap_train(cb, ds, p, qerror_out, false, "somhip_som_batchmap");
} ABI_CATCH(somhip_som_batchmap)
extern "C" int somhip_som_batchmap_missing(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p, float *qerror_out) try {
  return batchmap_train(cb, ds, p, qerror_out, true, "somhip_som_batchmap_missing");
} ABI_CATCH(somhip_som_batchmap_missing)

extern "C" int somhip_debug_batchmap_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, uint32_t *hits, double *sums) try {
  CHK(check_pair(cb, ds, "somhip_debug_batchmap_sums"));
  if (!hits || !sums) return fail("somhip_debug_batchmap_sums: null output");
  CHK(batchmap_check_codebook(cb, "somhip_debug_batchmap_sums"));
  CHK(batchmap_check_data(ds, first, n, "somhip_debug_batchmap_sums"));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  BatchmapBufs b;
  CHK(batchmap_bind(cb, n, &b));
  CHK(batchmap_sums_stage(cb, ds, first, n, b, nullptr));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  std::vector<double> hs(units * (d + 1));
  CHK(to_host(e, hits, b.hits, units));
  CHK(to_host_sync(e, hs.data(), b.S, hs.size()));
  split_trailing(hs.data(), units, d, sums, nullptr);
  return 0;
} ABI_CATCH(somhip_debug_batchmap_sums)

extern "C" int somhip_debug_batchmap_combine(somhip_codebook *cb, float r, const uint32_t *hits, const double *sums) try {
  CHK(check_codebook(cb, hits && sums, "somhip_debug_batchmap_combine"));
  CHK(batchmap_check_codebook(cb, "somhip_debug_batchmap_combine"));
  if (!(r >= 0.0f)) return fail("somhip_debug_batchmap_combine: radius %g < 0", (double)r);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  close_accumulations(cb);
  BatchmapBufs b;
  CHK(batchmap_bind(cb, 0, &b));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  std::vector<double> hs(units * (d + 1));
  for (size_t u = 0; u < units; u++) {
    memcpy(hs.data() + u * (d + 1), sums + u * d, sizeof(double) * d);
    hs[u * (d + 1) + d] = (double)hits[u];
  }
  CHK(to_device(e, b.S, hs.data(), hs.size()));
  CHK(batchmap_combine_stage(cb, r, b));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (hs is read until the copy has run)
  return 0;
} ABI_CATCH(somhip_debug_batchmap_combine)

// ... and the two stages of the missing form: sums and counts are [units][dim] each on the host, interleaved per unit in S
extern "C" int somhip_debug_batchmap_missing_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, double *sums,
                                                  double *counts) try {
  CHK(check_pair(cb, ds, "somhip_debug_batchmap_missing_sums"));
  if (!sums || !counts) return fail("somhip_debug_batchmap_missing_sums: null output");
  CHK(batchmap_check_codebook(cb, "somhip_debug_batchmap_missing_sums"));
  CHK(batchmap_check_data(ds, first, n, "somhip_debug_batchmap_missing_sums", true));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  BatchmapBufs b;
  CHK(batchmap_bind(cb, n, &b, nullptr, true));
  CHK(batchmap_sums_stage(cb, ds, first, n, b, nullptr));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  std::vector<double> hs(units * 2 * d);
  CHK(to_host_sync(e, hs.data(), b.S, hs.size()));
  for (size_t u = 0; u < units; u++) {
    memcpy(sums + u * d, hs.data() + u * 2 * d, sizeof(double) * d);
    memcpy(counts + u * d, hs.data() + u * 2 * d + d, sizeof(double) * d);
  }
  return 0;
} ABI_CATCH(somhip_debug_batchmap_missing_sums)

extern "C" int somhip_debug_batchmap_missing_combine(somhip_codebook *cb, float r, const double *sums, const double *counts) try {
  CHK(check_codebook(cb, sums && counts, "somhip_debug_batchmap_missing_combine"));
  CHK(batchmap_check_codebook(cb, "somhip_debug_batchmap_missing_combine"));
  if (!(r >= 0.0f)) return fail("somhip_debug_batchmap_missing_combine: radius %g < 0", (double)r);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  close_accumulations(cb);
  BatchmapBufs b;
  CHK(batchmap_bind(cb, 0, &b, nullptr, true));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  std::vector<double> hs(units * 2 * d);
  for (size_t u = 0; u < units; u++) {
    memcpy(hs.data() + u * 2 * d, sums + u * d, sizeof(double) * d);
    memcpy(hs.data() + u * 2 * d + d, counts + u * d, sizeof(double) * d);
  }
  CHK(to_device(e, b.S, hs.data(), hs.size()));
  CHK(batchmap_combine_stage(cb, r, b));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (hs is read until the copy has run)
  return 0;
} ABI_CATCH(somhip_debug_batchmap_missing_combine)

// HIP-event totals of the batch map's stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own
// behind the published table): [0] group (winners pass, scan, sort), [1] k_batchmap_sums, [2] the combine (with the
// gaussian table)
extern "C" int somhip_batchmap_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]) try {
  const int kid[3] = {KID_BATCHMAP_GROUP, KID_BATCHMAP_SUMS, KID_BATCHMAP_COMBINE};
  return stage_timing(e, "somhip_batchmap_timing", kid, 3, launches, total_ms);
} ABI_CATCH(somhip_batchmap_timing)

// ---------------------------------------------------------------------------------
// The epoch over data in pieces.  The state is one device blob the codebook owns: [S | counts] as units x (dim + 1)
// doubles, then the tail -- find_qerror's float so far and the samples taken.  Nothing of an accumulation lives on the
// host between calls, so the blob copied into another codebook of the same shape (its own state opened by _begin)
// continues there: that is what hands a chain from rank to rank.
// ---------------------------------------------------------------------------------
struct BatchmapTail { float q; uint32_t unused; uint64_t samples; };
static_assert(sizeof(BatchmapTail) == 16, "the tail of the batch map's state is two words of 8 bytes");
// (the form is that of the state the codebook holds: cb->bm_missing)
static size_t batchmap_state_doubles(const somhip_codebook *cb) { return (size_t)cb->v.n * batchmap_unit_doubles(cb, cb->bm_missing); }
static size_t batchmap_state_bytes(const somhip_codebook *cb) { return sizeof(double) * batchmap_state_doubles(cb) + sizeof(BatchmapTail); }
static BatchmapTail *batchmap_tail(const somhip_codebook *cb) { return reinterpret_cast<BatchmapTail *>(cb->bm_state + batchmap_state_doubles(cb)); }

// opens the state as all +0.0 (bits of zero throughout, the tail included).  A codebook holds one state, of one form: a
// state of the other form is given up here, so opening one form closes the other.
static int batchmap_state_open(somhip_codebook *cb, bool missing = false) {
  somhip_engine *e = cb->e;
  if (cb->bm_state && cb->bm_missing != missing) {
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipFree(cb->bm_state));
    cb->bm_state = nullptr;                                             // (open and moved are set below)
  }
  cb->bm_missing = missing;
  if (!cb->bm_state) HIPCHK(hipMalloc((void **)&cb->bm_state, batchmap_state_bytes(cb)));
  HIPCHK(hipMemsetAsync(cb->bm_state, 0, batchmap_state_bytes(cb), e->stream));
  cb->bm_open = true;
  cb->bm_moved = false;
  return 0;
}
static int batchmap_check_open(const somhip_codebook *cb, const char *who, bool missing = false) {
  if (!(cb->bm_open && cb->bm_state))
    return fail("%s: no accumulation is open on this codebook (%s first; a call that writes the rows closes it)", who,
                missing ? "somhip_batchmap_missing_begin" : "somhip_batchmap_begin");
  if (cb->bm_missing != missing)
    return fail("%s: the open accumulation has the other form, %s (it is continued by the somhip_batchmap_%s* calls)", who,
                cb->bm_missing ? "[S | C] of somhip_batchmap_missing_begin" : "[S | hits] of somhip_batchmap_begin", cb->bm_missing ? "missing_" : "");
  return 0;
}
// The tail as the pieces so far left it, and the refusal of a piece of n samples that would take the total to 2^32: a copy
// and a comparison, before anything is bound or launched.
static int batchmap_read_tail(somhip_codebook *cb, int64_t n, const char *who, BatchmapTail *tail) {
  CHK(to_host_sync(cb->e, tail, batchmap_tail(cb), 1));
  if (tail->samples + (uint64_t)n >= (uint64_t)1 << 32)
    return fail("%s: %llu + %lld samples do not fit the 32-bit hit counts", who, (unsigned long long)tail->samples, (long long)n);
  return 0;
}
// One piece into the open state, whose tail the caller has just read: the chains, the counts and the tail go on, the tail
// is written back.  dist (or null): the piece's group stage has run already (batchmap_group_stage with keep) and these are
// its distances.
static int batchmap_take_piece(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const BatchmapBufs &b, bool want_q,
                               const std::vector<float> *dist, BatchmapTail tail) {
  somhip_engine *e = cb->e;
  if (dist) { if (want_q) for (float d1 : *dist) if (!(d1 < 0.0f)) batchmap_q_step(tail.q, d1); }
  else CHK(batchmap_group_stage(cb, ds, first, n, b, want_q ? &tail.q : nullptr));
  CHK(batchmap_sums_launch(cb, ds, first, b, true));
  tail.samples += (uint64_t)n;
  CHK(to_device(e, batchmap_tail(cb), &tail, 1));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (tail is read until the copy has run)
  return 0;
}

// The five calls of either form (missing: the state is [S | C] and the pieces may carry masks), each one body
static int batchmap_begin(somhip_codebook *cb, bool missing, const char *who) {
  CHK(check_codebook(cb, true, who));
  CHK(batchmap_check_codebook(cb, who));
  HIPCHK(hipSetDevice(cb->e->device));
  CHK(batchmap_state_open(cb, missing));
  HIPCHK(hipStreamSynchronize(cb->e->stream));
  return 0;
}
static int batchmap_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int want_qerror, bool missing,
                               const char *who) {
  CHK(check_pair(cb, ds, who));
  CHK(batchmap_check_codebook(cb, who));
  CHK(batchmap_check_data(ds, first, n, who, missing));
  CHK(batchmap_check_open(cb, who, missing));
  if (cb->bm_moved)
    return fail("%s: the codebook has moved (somhip_batchmap_%sfinish has run; somhip_batchmap_%sbegin opens the next epoch)", who,
                missing ? "missing_" : "", missing ? "missing_" : "");
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  BatchmapTail tail;
  CHK(batchmap_read_tail(cb, n, who, &tail));                           // (the last refusal: nothing is bound before it)
  BatchmapBufs b;
  CHK(batchmap_bind(cb, n, &b, cb->bm_state, missing));
  return batchmap_take_piece(cb, ds, first, n, b, want_qerror != 0, nullptr, tail);
}
// _finish is one body too, and it is somhip_batchmap_finish's own: the one owner of a batch-map state that updates the rows
// from it and re-opens it behind the combine.  somhip_batchmap_missing_finish runs that body and says so here, for the
// calling thread: the name the refusals go by, null for the plain call.
static thread_local const char *bm_finish_as = nullptr;
extern "C" int somhip_batchmap_finish(somhip_codebook *cb, float r, int64_t group_first, int64_t group_count, float *qerror_out) try {
  const bool missing = bm_finish_as != nullptr;
  const char *who = missing ? bm_finish_as : "somhip_batchmap_finish";
  CHK(check_codebook(cb, true, who));
  CHK(batchmap_check_codebook(cb, who));
  CHK(batchmap_check_open(cb, who, missing));
  if (!(r >= 0.0f)) return fail("%s: radius %g < 0", who, (double)r);
  if (group_first < 0 || group_count < 0 || group_first > cb->v.ngroups || group_count > cb->v.ngroups - group_first)
    return fail("%s: row groups [%lld, +%lld) outside [0, %lld]", who, (long long)group_first, (long long)group_count,
                (long long)cb->v.ngroups);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  BatchmapBufs b;
  CHK(batchmap_bind(cb, 0, &b, cb->bm_state, missing));
  if (group_count > 0) cb->bm_moved = true;                             // (an empty range writes no row)
  const int rc = batchmap_combine_stage(cb, r, b, group_first, group_count);
  cb->bm_open = true;                                                   // (the combine closes every accumulation; this one stays,
  CHK(rc);                                                              //  also where a launch of the combine failed)
  BatchmapTail tail{};
  if (qerror_out) CHK(to_host(e, &tail, batchmap_tail(cb), 1));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (qerror_out) *qerror_out = tail.q;
  return 0;
} ABI_CATCH(somhip_batchmap_finish)
// (_end frees the state whichever form it has: there is one)
static int batchmap_end(somhip_codebook *cb, const char *who) {
  CHK(check_codebook(cb, true, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (cb->bm_state) HIPCHK(hipFree(cb->bm_state));
  cb->bm_state = nullptr;
  cb->bm_open = cb->bm_moved = false;
  return 0;
}
static int batchmap_state(somhip_codebook *cb, void **dev_state, int64_t *bytes, bool missing, const char *who) {
  CHK(check_codebook(cb, dev_state && bytes, who));
  CHK(batchmap_check_open(cb, who, missing));
  *dev_state = cb->bm_state;
  *bytes = (int64_t)batchmap_state_bytes(cb);
  return 0;
}

extern "C" int somhip_batchmap_begin(somhip_codebook *cb) try {
  return batchmap_begin(cb, false, "somhip_batchmap_begin");
} ABI_CATCH(somhip_batchmap_begin)
extern "C" int somhip_batchmap_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int want_qerror) try {
  return batchmap_accumulate(cb, ds, first, n, want_qerror, false, "somhip_batchmap_accumulate");
} ABI_CATCH(somhip_batchmap_accumulate)
extern "C" int somhip_batchmap_end(somhip_codebook *cb) try {
  return batchmap_end(cb, "somhip_batchmap_end");
} ABI_CATCH(somhip_batchmap_end)
extern "C" int somhip_batchmap_state(somhip_codebook *cb, void **dev_state, int64_t *bytes) try {
  return batchmap_state(cb, dev_state, bytes, false, "somhip_batchmap_state");
} ABI_CATCH(somhip_batchmap_state)

extern "C" int somhip_batchmap_missing_begin(somhip_codebook *cb) try {
  return batchmap_begin(cb, true, "somhip_batchmap_missing_begin");
} ABI_CATCH(somhip_batchmap_missing_begin)
extern "C" int somhip_batchmap_missing_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int want_qerror) try {
  return batchmap_accumulate(cb, ds, first, n, want_qerror, true, "somhip_batchmap_missing_accumulate");
} ABI_CATCH(somhip_batchmap_missing_accumulate)
extern "C" int somhip_batchmap_missing_finish(somhip_codebook *cb, float r, int64_t group_first, int64_t group_count, float *qerror_out) try {
  struct As {
    As() { bm_finish_as = "somhip_batchmap_missing_finish"; }
    ~As() { bm_finish_as = nullptr; }
  } as;
  return somhip_batchmap_finish(cb, r, group_first, group_count, qerror_out);
} ABI_CATCH(somhip_batchmap_missing_finish)
extern "C" int somhip_batchmap_missing_end(somhip_codebook *cb) try {
  return batchmap_end(cb, "somhip_batchmap_missing_end");
} ABI_CATCH(somhip_batchmap_missing_end)
extern "C" int somhip_batchmap_missing_state(somhip_codebook *cb, void **dev_state, int64_t *bytes) try {
  return batchmap_state(cb, dev_state, bytes, true, "somhip_batchmap_missing_state");
} ABI_CATCH(somhip_batchmap_missing_state)

// The epochs of somhip_som_batchmap over the row blocks of the communicator's ranks, block by block in rank order.  Every
// rank holds the whole map.  Per epoch: the group stage on every rank's own block at once (the search); then, rank after
// rank, the continued sums and the q chain on the rank whose turn it is, and the state broadcast from it; the combine of
// the rank's share of the row groups; an all-gather of the shares' tile ranges.
extern "C" int somhip_som_batchmap_ranks(somhip_codebook *cb, somhip_dataset *block, const somhip_batchmap_params *p, somhip_comm *c,
                                         float *qerror_out) try {
  const char *who = "somhip_som_batchmap_ranks";
  CHK(check_codebook(cb, p && c, who));
  const bool empty = p->n == 0;                                          // a rank whose block holds no row: legal here and only here
  if (!empty) CHK(check_pair(cb, block, who));
  CHK(batchmap_check_codebook(cb, who));
  if (!empty) CHK(batchmap_check_data(block, p->first, p->n, who));
  if (c->e != cb->e) return fail("%s: codebook and communicator belong to different engines", who);
  CHK(check_epochs(p->epochs, who));
  if (!(p->radius >= 1.0f)) return fail("%s: radius %g < 1", who, (double)p->radius);
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const int64_t ngroups = cb->v.ngroups, share = (ngroups + c->world - 1) / c->world;
  const int64_t g0 = std::min<int64_t>((int64_t)c->rank * share, ngroups), gn = std::min<int64_t>(share, ngroups - g0);
  const size_t group_floats = (size_t)cb->v.d4 * WAVE * 4;              // a row group's tiles: one contiguous range of cb.tiles
  struct Staging {
    float *send = nullptr, *recv = nullptr;
    uint32_t *words = nullptr;
    ~Staging() { if (send) (void)hipFree(send); if (recv) (void)hipFree(recv); if (words) (void)hipFree(words); }
  } st;
  // The blocks' rows together must fit the 32-bit hit counts: every rank learns the total (summed as two 16-bit halves, so
  // the words cannot overflow) and refuses alike, before any rank has launched anything.
  HIPCHK(hipMalloc((void **)&st.words, 2 * sizeof(uint32_t)));
  uint32_t halves[2] = {(uint32_t)(p->n >> 16), (uint32_t)(p->n & 0xffff)};
  CHK(to_device(e, st.words, halves, 2));
  HIPCHK(hipStreamSynchronize(e->stream));
  CHK(somhip_comm_allreduce_sum_u32(c, st.words, 2));
  CHK(to_host_sync(e, halves, st.words, 2));
  const uint64_t total = ((uint64_t)halves[0] << 16) + halves[1];
  if (total >= (uint64_t)1 << 32) return fail("%s: the ranks' %llu samples do not fit the 32-bit hit counts", who, (unsigned long long)total);
  HIPCHK(hipMalloc((void **)&st.send, sizeof(float) * group_floats * (size_t)share));
  HIPCHK(hipMalloc((void **)&st.recv, sizeof(float) * group_floats * (size_t)share * (size_t)c->world));
  HIPCHK(hipMemsetAsync(st.send, 0, sizeof(float) * group_floats * (size_t)share, e->stream));     // (the last share's padding)
  auto epochs = [&]() -> int {
    BatchmapBufs b;
    std::vector<float> dist;
    for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
      const float r = 1.0f + linear_rate(p->radius - 1.0f, p->epochs, t);
      float *q = qerror_out ? qerror_out + (t - p->start_epoch) : nullptr;
      CHK(batchmap_state_open(cb));
      b = BatchmapBufs();
      CHK(batchmap_bind(cb, p->n, &b, cb->bm_state));
      float unused = 0.0f;
      if (!empty) CHK(batchmap_group_stage(cb, block, p->first, p->n, b, q ? &unused : nullptr, &dist));
      for (int root = 0; root < c->world; root++) {
        if (root == c->rank && !empty) {
          BatchmapTail tail;
          CHK(batchmap_read_tail(cb, p->n, who, &tail));
          CHK(batchmap_take_piece(cb, block, p->first, p->n, b, q != nullptr, &dist, tail));
        }
        CHK(somhip_comm_broadcast(c, cb->bm_state, (int64_t)batchmap_state_bytes(cb), root));
      }
      CHK(batchmap_combine_stage(cb, r, b, g0, gn));
      if (gn > 0) CHK(on_device(e, st.send, cb->v.tiles + group_floats * (size_t)g0, group_floats * (size_t)gn));
      CHK(somhip_comm_allgather(c, st.send, st.recv, (int64_t)(sizeof(float) * group_floats * (size_t)share)));
      CHK(on_device(e, cb->v.tiles, st.recv, group_floats * (size_t)ngroups));   // (shares are consecutive: the gathered ranges are the tiles)
      rows_written(cb);
      if (q) {
        BatchmapTail tail;
        CHK(to_host_sync(e, &tail, batchmap_tail(cb), 1));
        *q = tail.q;
      }
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
  };
  const int rc = epochs();
  // The state was the epochs' own, on every way out: closed, so that no later _finish combines a state that was broadcast
  // half way, and freed (units x (dim + 1) doubles are not kept for a codebook that may never accumulate again).
  (void)hipStreamSynchronize(e->stream);
  if (cb->bm_state) (void)hipFree(cb->bm_state);
  cb->bm_state = nullptr;
  cb->bm_open = cb->bm_moved = false;
  return rc;
} ABI_CATCH(somhip_som_batchmap_ranks)
