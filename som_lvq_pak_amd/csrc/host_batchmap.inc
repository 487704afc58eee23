// host_batchmap.inc -- K8, the batch map: per epoch the winners of every sample against the frozen codebook, the per-unit
// ordered fp64 sums (stage 1) and the neighbourhood combine on the fp64 MFMA (stage 2)
// (included by somhip.hip: one translation unit, shared static helpers)
#include <rocprim/device/device_radix_sort.hpp>

// The device arrays of a batch-map call.  SLOT_BATCHMAP, per unit: [S: units x (dim + 1) doubles][the gaussian table]
// [hits][starts: units + 1].  SLOT_BATCHMAP_LIST, per sample: [win][idx][the sorted winners][list][the sort's own room].
struct BatchmapBufs {
  double *S = nullptr, *table = nullptr;
  uint32_t *hits = nullptr, *starts = nullptr, *win = nullptr, *idx = nullptr, *win_sorted = nullptr, *list = nullptr;
  void *sort_tmp = nullptr;
  size_t sort_bytes = 0;
  unsigned sort_bits = 0;             // the winners' bits that differ: those of 0 .. units
};
static size_t batchmap_table_len(const somhip_codebook *cb) {
  return cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN ? 2 * (size_t)(2 * cb->v.xdim - 1) * (size_t)(2 * cb->ydim - 1) : 0;
}
// n: the samples of a sums stage, 0 where only the combine runs
static int batchmap_bind(somhip_codebook *cb, int64_t n, BatchmapBufs *b) {
  somhip_engine *e = cb->e;
  const size_t units = (size_t)cb->v.n, ns = (size_t)n, s_len = units * (size_t)(cb->v.d + 1), t_len = batchmap_table_len(cb);
  void *p;
  CHK(engine_scratch(e, SLOT_BATCHMAP, sizeof(double) * (s_len + t_len) + sizeof(uint32_t) * (2 * units + 1), &p));
  b->S = (double *)p;
  b->table = b->S + s_len;
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

// Stage 1 (steps 2-3 of the definition, include/somhip.h): b.S <- [S | hits], b.hits <- hits, of data rows (first + s) %
// n_rows, s < n, against the codebook as it stands.  Per chunk (knn_chunk_keys with knn 1, SOMHIP_TIE_FIRST): the keys,
// k_batchmap_winners behind them; then the scan, the stable sort by winner and the sums.  qerror (or null: no per-sample
// copy leaves the device): find_qerror's float chain over the winners' distances in data order, as somhip_map_quality forms it.
static int batchmap_sums_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const BatchmapBufs &b, float *qerror) {
  somhip_engine *e = cb->e;
  const uint32_t units = (uint32_t)cb->v.n;
  HIPCHK(hipMemsetAsync(b.hits, 0, sizeof(uint32_t) * (size_t)units, e->stream));
  float q = 0.0f;
  std::vector<float> hd;
  CHK(knn_chunk_keys(cb, ds, first, n, 1, 0, [&](int64_t off, int64_t f, int64_t c, const uint64_t *dk, int stride) {
    float *dd1 = nullptr;
    if (qerror) CHK(scratch(e, SLOT_CALL_B, (size_t)c, &dd1));
    CHK(LAUNCH_TIMED(e, KID_BATCHMAP_GROUP, k_batchmap_winners, dim3((unsigned)((c + BM_THREADS - 1) / BM_THREADS)), dim3(BM_THREADS), 0, dk,
        stride, off, c, units, b.win, b.idx, dd1, b.hits));
    if (!qerror) return 0;
    if (hd.empty()) hd.resize((size_t)c);                               // (the first chunk is the longest)
    CHK(to_host_sync(e, hd.data(), dd1, (size_t)c));
    for (int64_t i = 0; i < c; i++) {
      if (sample_is_empty(ds, (f + i) % ds->n)) continue;               // ignore empty vectors, som_rout.c:712
      q += sqrt((double)hd[(size_t)i]);                                 // float accumulator, :715
    }
    return 0;
  }));
  CHK(LAUNCH_TIMED(e, KID_BATCHMAP_GROUP, k_batchmap_starts, dim3(1), dim3(BM_SCAN_THREADS), 0, b.hits, units, b.starts));
  {
    LaunchTimer t(e, KID_BATCHMAP_GROUP);                               // (rocPRIM's own launches, on the engine's stream)
    size_t bytes = b.sort_bytes;
    const hipError_t er = rocprim::radix_sort_pairs(b.sort_tmp, bytes, b.win, b.win_sorted, b.idx, b.list, (size_t)n, 0u, b.sort_bits, e->stream);
    if (er != hipSuccess) return fail("batch map: the sort by winner failed: %s", hipGetErrorString(er));
  }
  CHK(LAUNCH_TIMED(e, KID_BATCHMAP_SUMS, k_batchmap_sums, dim3(units, (unsigned)((cb->v.d + 1 + BM_SUM_DIMS - 1) / BM_SUM_DIMS)), dim3(BM_SUM_DIMS), 0,
      ds->d_rows, ds->n, ds->d, first % ds->n, b.list, b.starts, b.S));
  if (qerror) *qerror = q;
  return 0;
}

// Stage 2 (steps 4-5): the codebook's rows <- (float)(N / D) from b.S at radius r, where D > 0.
static int batchmap_combine_stage(somhip_codebook *cb, float r, const BatchmapBufs &b) {
  somhip_engine *e = cb->e;
  const bool gauss = cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN;
  const int small_map = cb->v.xdim <= 1024 && cb->ydim <= 1024;         // (lattice_sq_small's condition)
  const dim3 grid((unsigned)cb->v.ngroups, (unsigned)((cb->v.d + BM_COLS - 1) / BM_COLS));
  cb->prep_valid = false;
  if (gauss) {
    const size_t t_len = batchmap_table_len(cb);
    CHK(LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_gauss_table, dim3((unsigned)((t_len + BM_THREADS - 1) / BM_THREADS)), dim3(BM_THREADS), 0,
        cb->v.topol, cb->v.xdim, cb->ydim, r, b.table));
    return LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_combine<true>, grid, dim3(256), 0, cb->v, cb->ydim, b.S, r, small_map, b.table);
  }
  return LAUNCH_TIMED(e, KID_BATCHMAP_COMBINE, k_batchmap_combine<false>, grid, dim3(256), 0, cb->v, cb->ydim, b.S, bubble_threshold(r), small_map,
                      nullptr);
}

// what every batch-map entry point refuses before anything is launched
static int batchmap_check_codebook(const somhip_codebook *cb, const char *who) {
  if (is_shard(cb)) return fail("%s: sharded codebook not supported (a shard does not hold the other shards' units)", who);
  if ((cb->v.topol != SOMHIP_TOPOL_HEXA && cb->v.topol != SOMHIP_TOPOL_RECT) || (int64_t)cb->v.xdim * cb->ydim != cb->v.n)
    return fail("%s: codebook without a lattice (%d x %d units, %lld rows)", who, cb->v.xdim, cb->ydim, (long long)cb->v.n);
  if (cb->v.neigh != SOMHIP_NEIGH_BUBBLE && cb->v.neigh != SOMHIP_NEIGH_GAUSSIAN) return fail("%s: unknown neighbourhood %d", who, cb->v.neigh);
  return 0;
}
static int batchmap_check_data(const somhip_dataset *ds, int64_t first, int64_t n, const char *who) {
  if (ds->d_mask) return fail("%s: data with masked components (x) is not supported", who);
  if (first < 0) return fail("%s: first row %lld < 0", who, (long long)first);
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  if (n >= (int64_t)1 << 32) return fail("%s: n %lld does not fit the 32-bit hit counts", who, (long long)n);
  return 0;
}

extern "C" int somhip_som_batchmap(somhip_codebook *cb, somhip_dataset *ds, const somhip_batchmap_params *p, float *qerror_out) try {
  CHK(check_pair(cb, ds, "somhip_som_batchmap"));
  if (!p) return fail("somhip_som_batchmap: null parameters");
  CHK(batchmap_check_codebook(cb, "somhip_som_batchmap"));
  CHK(batchmap_check_data(ds, p->first, p->n, "somhip_som_batchmap"));
  if (p->epochs < 1) return fail("somhip_som_batchmap: epochs %lld < 1", (long long)p->epochs);
  if (!(p->radius >= 1.0f)) return fail("somhip_som_batchmap: radius %g < 1", (double)p->radius);
  if (p->start_epoch < 0 || p->count < 0 || p->start_epoch + p->count > p->epochs)
    return fail("somhip_som_batchmap: epochs [%lld, %lld) outside [0, %lld)", (long long)p->start_epoch, (long long)(p->start_epoch + p->count),
                (long long)p->epochs);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  BatchmapBufs b;
  CHK(batchmap_bind(cb, p->n, &b));
  const float T = (float)p->epochs;
  for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
    const float r = 1.0f + (p->radius - 1.0f) * (float)(p->epochs - t) / T;   // som_rout.c:615 over epochs
    CHK(batchmap_sums_stage(cb, ds, p->first, p->n, b, qerror_out ? qerror_out + (t - p->start_epoch) : nullptr));
    CHK(batchmap_combine_stage(cb, r, b));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_som_batchmap)

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
  for (size_t u = 0; u < units; u++) memcpy(sums + u * d, hs.data() + u * (d + 1), sizeof(double) * d);
  return 0;
} ABI_CATCH(somhip_debug_batchmap_sums)

extern "C" int somhip_debug_batchmap_combine(somhip_codebook *cb, float r, const uint32_t *hits, const double *sums) try {
  CHK(check_codebook(cb, hits && sums, "somhip_debug_batchmap_combine"));
  CHK(batchmap_check_codebook(cb, "somhip_debug_batchmap_combine"));
  if (!(r >= 0.0f)) return fail("somhip_debug_batchmap_combine: radius %g < 0", (double)r);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
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

// HIP-event totals of the batch map's stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own
// behind the published table): [0] group (winners pass, scan, sort), [1] k_batchmap_sums, [2] the combine (with the
// gaussian table)
extern "C" int somhip_batchmap_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]) try {
  CHK(check_engine(e, "somhip_batchmap_timing"));
  if (!launches || !total_ms) return fail("somhip_batchmap_timing: null output");
  CHK(timing_flush(e));
  const int kid[3] = {KID_BATCHMAP_GROUP, KID_BATCHMAP_SUMS, KID_BATCHMAP_COMBINE};
  for (int i = 0; i < 3; i++) { launches[i] = e->launches[kid[i]]; total_ms[i] = e->total_ms[kid[i]]; }
  return 0;
} ABI_CATCH(somhip_batchmap_timing)
