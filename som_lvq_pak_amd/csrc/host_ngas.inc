// host_ngas.inc -- K10, batch neural gas: per epoch the schedule (host, double), the K nearest units of every sample against
// the frozen codebook (the engine's k-NN search), the (unit, sample, rank) entries grouped by unit, the per-unit ordered
// fp64 sums of rank-weighted rows and the update; the stages on their own for the tests
// (included by somhip.hip behind host_glvq.inc: one translation unit, the trainers' shared checks and the trailing column
// of host_proto.inc, K8's scan of the counts, rocPRIM's sort)

// The segment rule, stated once.  The data go through the entries, the sort and the sums in segments of consecutive
// samples; a segment holds at most NG_SEGMENT_PAIRS (sample, rank) pairs, so the sort's buffers stay bounded (16 bytes a
// pair and the sort's own room: about 0.4 GiB) whatever n is, and at most 2^24 samples, the sample field of a packed
// list value.  It is a whole number of the search's 4096-sample chunks where more than one chunk fits (K <= 256: at
// least 16 of them), and never longer than the data set, so that a segment's rows wrap at most once (k_ng_sums wraps by
// one select; a run over more samples than the data set has rows takes more segments).  The segments after the first
// continue the chains, so the result does not depend on the rule; a caller's own segment length (somhip_debug_ng_sums)
// is taken as given, below the same bounds.
constexpr int64_t NG_SEGMENT_PAIRS = (int64_t)1 << 24;
constexpr int64_t NG_SEARCH_CHUNK = 4096;
constexpr double NG_RANK_REACH = 17.0;          // ranks at and beyond 1 + floor(17 lambda) weigh less than exp(-17) < 2^-24
static int64_t ng_segment(int K, int64_t wanted) {
  const int64_t most = NG_SEGMENT_PAIRS / K;    // (K <= 256: at least 65536 samples, at most 2^24)
  if (wanted > 0) return std::min(wanted, most);
  return most / NG_SEARCH_CHUNK * NG_SEARCH_CHUNK;
}

// Step 1 of the definition (include/somhip.h), in double on the host: lambda_t, K_t and the weights of epoch t; w[256], zeros
// behind K_t.
static void ng_schedule(const somhip_ng_params &p, int64_t units, int64_t t, double *lambda, int *K, double *w) {
  double lam = p.lambda0;
  if (p.epochs > 1) {
    const double ratio = p.lambda_end / p.lambda0, frac = (double)t / (double)(p.epochs - 1);
    lam = p.lambda0 * pow(ratio, frac);
  }
  int k = (int)p.ranks;
  if (k <= 0) {
    const double cap = (double)std::min<int64_t>(units, SOMHIP_KNN_MAX), reach = 1.0 + floor(NG_RANK_REACH * lam);
    k = (int)(reach < cap ? reach : cap);
  }
  for (int r = 0; r < SOMHIP_KNN_MAX; r++) w[r] = r < k ? exp(-(double)r / lam) : 0.0;
  *lambda = lam;
  *K = k;
}

// The device arrays of a neural-gas call.  SLOT_NGAS, per unit: [S | W: units x (dim + 1) doubles][w: SOMHIP_KNN_MAX doubles]
// [hits: the lists' lengths over all segments][seg_hits: a segment's][starts: units + 1].  SLOT_NGAS_LIST, per pair of a
// segment: [unit][packed][the sorted units][list][the sort's own room].
struct NgBufs {
  double *S = nullptr, *w = nullptr;
  uint32_t *hits = nullptr, *seg_hits = nullptr, *starts = nullptr;
  uint32_t *unit = nullptr, *packed = nullptr, *unit_sorted = nullptr, *list = nullptr;
  void *sort_tmp = nullptr;
  size_t sort_bytes = 0;
  unsigned sort_bits = 0;             // the units' bits that differ: those of 0 .. units
};
// pairs: the most pairs of a segment, 0 where only the update runs
static int ng_bind(somhip_codebook *cb, int64_t pairs, NgBufs *b) {
  somhip_engine *e = cb->e;
  const size_t units = (size_t)cb->v.n, np = (size_t)pairs, s_len = units * (size_t)(cb->v.d + 1);
  void *p;
  CHK(engine_scratch(e, SLOT_NGAS, sizeof(double) * (s_len + SOMHIP_KNN_MAX) + sizeof(uint32_t) * (3 * units + 1), &p));
  b->S = (double *)p;
  b->w = b->S + s_len;
  b->hits = reinterpret_cast<uint32_t *>(b->w + SOMHIP_KNN_MAX);
  b->seg_hits = b->hits + units;
  b->starts = b->seg_hits + units;
  if (pairs <= 0) return 0;
  for (size_t u = units; u; u >>= 1) b->sort_bits++;
  const hipError_t er = rocprim::radix_sort_pairs(nullptr, b->sort_bytes, b->unit, b->unit_sorted, b->packed, b->list, np, 0u, b->sort_bits, e->stream);
  if (er != hipSuccess) return fail("neural gas: the sort's size query failed: %s", hipGetErrorString(er));
  const size_t arrays = (sizeof(uint32_t) * 4 * np + 255) / 256 * 256;
  CHK(engine_scratch(e, SLOT_NGAS_LIST, arrays + b->sort_bytes, &p));
  b->unit = (uint32_t *)p;
  b->packed = b->unit + np;
  b->unit_sorted = b->packed + np;
  b->list = b->unit_sorted + np;
  b->sort_tmp = (char *)p + arrays;
  return 0;
}

// Step 2 over one segment -- the run's samples seg_off .. seg_off + seg_n - 1 -- and the grouping: per chunk of the search
// (knn_chunk_keys under find_winner_knn's order; K == 1 on two rows and more searches with knn 2 and leaves the second
// key unread, a one-row codebook searches with knn 1 and plain tags) the keys and k_ng_entries behind them; then the scan
// of the segment's counts and the stable sort of the pairs by unit.  q (or null: no per-sample copy leaves the device):
// find_qerror's float chain over the rank-0 distances in data order, continued.  keys_out (or null): the chunks' keys
// [seg_n][K] to the host, for the ranks stage.
static int ng_entries_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t seg_off, int64_t seg_n, int K, const NgBufs &b,
                            float *q, uint64_t *keys_out) {
  somhip_engine *e = cb->e;
  const uint32_t units = (uint32_t)cb->v.n;
  const int knn = K == 1 && units >= 2 ? 2 : K;
  HIPCHK(hipMemsetAsync(b.seg_hits, 0, sizeof(uint32_t) * (size_t)units, e->stream));
  std::vector<float> hd;
  std::vector<uint64_t> hk;
  CHK(knn_chunk_keys(cb, ds, first % ds->n + seg_off, seg_n, knn, 1, [&](int64_t off, int64_t f, int64_t c, const uint64_t *dk, int stride) {
    float *dd0 = nullptr;
    if (q) CHK(scratch(e, SLOT_CALL_B, (size_t)c, &dd0));
    CHK(LAUNCH_TIMED(e, KID_NG_GROUP, k_ng_entries, dim3((unsigned)((c * K + NG_THREADS - 1) / NG_THREADS)), dim3(NG_THREADS), 0, dk, stride, K,
        knn >= 2 ? 1 : 0, off, c, units, b.unit, b.packed, dd0, b.seg_hits));
    if (keys_out) {
      if (hk.empty()) hk.resize((size_t)c * stride);                    // (the first chunk is the longest)
      CHK(to_host_sync(e, hk.data(), dk, (size_t)c * stride));
      for (int64_t i = 0; i < c; i++) memcpy(keys_out + (size_t)(off + i) * K, hk.data() + (size_t)i * stride, sizeof(uint64_t) * (size_t)K);
    }
    if (!q) return 0;
    if (hd.empty()) hd.resize((size_t)c);
    CHK(to_host_sync(e, hd.data(), dd0, (size_t)c));
    for (int64_t i = 0; i < c; i++)
      if (!sample_is_empty(ds, (f + i) % ds->n)) batchmap_q_step(*q, hd[(size_t)i]);
    return 0;
  }));
  CHK(LAUNCH_TIMED(e, KID_NG_GROUP, k_batchmap_starts, dim3(1), dim3(BM_SCAN_THREADS), 0, b.seg_hits, units, b.starts));
  LaunchTimer t(e, KID_NG_GROUP);                                       // (rocPRIM's own launches, on the engine's stream)
  size_t bytes = b.sort_bytes;
  const hipError_t er = rocprim::radix_sort_pairs(b.sort_tmp, bytes, b.unit, b.unit_sorted, b.packed, b.list, (size_t)(seg_n * K), 0u, b.sort_bits,
                                                  e->stream);
  if (er != hipSuccess) return fail("neural gas: the sort by unit failed: %s", hipGetErrorString(er));
  return 0;
}
// Step 3 over the segment the entries stage has grouped: b.S and b.hits from the lists and b.w.  cont: not the run's first
// segment -- the chains and the counts go on from what b.S and b.hits hold.
static int ng_sums_launch(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t seg_off, const NgBufs &b, bool cont) {
  const dim3 grid((unsigned)cb->v.n, (unsigned)((cb->v.d + 1 + BM_SUM_DIMS - 1) / BM_SUM_DIMS));
  const int64_t f = (first % ds->n + seg_off) % ds->n;
  if (cont)
    return LAUNCH_TIMED(cb->e, KID_NG_SUMS, k_ng_sums<true>, grid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->n, ds->d, f, b.list, b.starts, b.w, b.S, b.hits);
  return LAUNCH_TIMED(cb->e, KID_NG_SUMS, k_ng_sums<false>, grid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->n, ds->d, f, b.list, b.starts, b.w, b.S, b.hits);
}
// Steps 2-3 of an epoch: every segment in turn, with the weights already in b.w
static int ng_sums_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int K, int64_t segment, const NgBufs &b, float *q) {
  segment = std::min(segment, ds->n);                                   // (the segment rule: k_ng_sums wraps a row once)
  for (int64_t off = 0; off < n; off += segment) {
    CHK(ng_entries_stage(cb, ds, first, off, std::min(segment, n - off), K, b, q, nullptr));
    CHK(ng_sums_launch(cb, ds, first, off, b, off > 0));
  }
  return 0;
}
// Step 4: the rows from b.S
static int ng_update_stage(somhip_codebook *cb, const NgBufs &b) {
  const int64_t threads = cb->v.ngroups * cb->v.d4 * WAVE;
  rows_written(cb);
  return LAUNCH_TIMED(cb->e, KID_NG_UPDATE, k_ng_update, dim3((unsigned)((threads + NG_THREADS - 1) / NG_THREADS)), dim3(NG_THREADS), 0, cb->v, b.S);
}

// what every neural-gas entry point refuses before anything is launched
static int ng_check_codebook(const somhip_codebook *cb, const char *who) {
  if (is_shard(cb)) return fail("%s: sharded codebook not supported (a shard does not hold the other shards' units)", who);
  return 0;
}
static int ng_check(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const char *who) {
  CHK(check_pair(cb, ds, who));
  CHK(ng_check_codebook(cb, who));
  if (ds->d_mask) return fail("%s: data with masked components (x) is not supported", who);
  if (first < 0) return fail("%s: first row %lld < 0", who, (long long)first);
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  if (n >= (int64_t)1 << 32) return fail("%s: n %lld does not fit the 32-bit hit counts", who, (long long)n);
  return 0;
}
static int ng_check_ranks(int64_t K, int least, const char *who) {
  return K >= least && K <= SOMHIP_KNN_MAX ? 0 : fail("%s: ranks %lld outside %d .. %d", who, (long long)K, least, SOMHIP_KNN_MAX);
}
static int ng_check_params(const somhip_ng_params *p, const char *who) {
  if (!p) return fail("%s: null parameters", who);
  CHK(check_epochs(p->epochs, who));
  if (!(p->lambda0 > 0.0) || std::isinf(p->lambda0)) return fail("%s: lambda0 %g is not a positive number", who, p->lambda0);
  if (!(p->lambda_end > 0.0) || !(p->lambda_end <= p->lambda0))
    return fail("%s: lambda_end %g outside (0, lambda0 = %g]", who, p->lambda_end, p->lambda0);
  return ng_check_ranks(p->ranks, 0, who);
}

extern "C" int somhip_debug_ng_schedule(const somhip_ng_params *p, int64_t units, int64_t t, double *lambda, int32_t *K, double *weights) try {
  const char *who = "somhip_debug_ng_schedule";
  CHK(ng_check_params(p, who));
  if (!lambda || !K || !weights) return fail("%s: null output", who);
  if (units < 1) return fail("%s: units %lld < 1", who, (long long)units);
  if (t < 0 || t >= p->epochs) return fail("%s: epoch %lld outside [0, %lld)", who, (long long)t, (long long)p->epochs);
  int k = 0;
  ng_schedule(*p, units, t, lambda, &k, weights);
  *K = k;
  return 0;
} ABI_CATCH(somhip_debug_ng_schedule)

extern "C" int somhip_ng_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_ng_params *p, float *qerror_out) try {
  const char *who = "somhip_ng_train";
  if (!cb || !ds) return fail("%s: null handle", who);
  CHK(ng_check_params(p, who));
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  CHK(ng_check(cb, ds, p->first, p->n, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  close_accumulations(cb);
  const int64_t units = cb->v.n;
  // the schedule of every epoch of the call, before the first launch: the tables are read until their copies have run
  std::vector<double> w((size_t)p->count * SOMHIP_KNN_MAX);
  std::vector<int> K((size_t)p->count);
  int64_t pairs = 0;
  for (int64_t i = 0; i < p->count; i++) {
    double lambda;
    ng_schedule(*p, units, p->start_epoch + i, &lambda, &K[(size_t)i], w.data() + (size_t)i * SOMHIP_KNN_MAX);
    pairs = std::max(pairs, std::min(p->n, ng_segment(K[(size_t)i], 0)) * K[(size_t)i]);
  }
  NgBufs b;
  CHK(ng_bind(cb, pairs, &b));
  for (int64_t i = 0; i < p->count; i++) {
    float q = 0.0f;
    CHK(to_device(e, b.w, w.data() + (size_t)i * SOMHIP_KNN_MAX, SOMHIP_KNN_MAX));
    CHK(ng_sums_stage(cb, ds, p->first, p->n, K[(size_t)i], ng_segment(K[(size_t)i], 0), b, qerror_out ? &q : nullptr));
    if (qerror_out) qerror_out[i] = q;
    CHK(ng_update_stage(cb, b));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_ng_train)

extern "C" int somhip_debug_ng_ranks(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int K, int32_t *units_out,
                                     float *dist_out) try {
  const char *who = "somhip_debug_ng_ranks";
  if (!units_out || !dist_out) return fail("%s: null output", who);
  CHK(ng_check_ranks(K, 1, who));
  CHK(ng_check(cb, ds, first, n, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const int64_t segment = ng_segment(K, 0);
  NgBufs b;
  CHK(ng_bind(cb, std::min(n, segment) * K, &b));
  std::vector<uint64_t> hk((size_t)(std::min(n, segment) * K));
  std::vector<uint32_t> hu(hk.size());
  for (int64_t off = 0; off < n; off += segment) {
    const int64_t c = std::min(segment, n - off);
    CHK(ng_entries_stage(cb, ds, first, off, c, K, b, nullptr, hk.data()));
    CHK(to_host_sync(e, hu.data(), b.unit, (size_t)(c * K)));           // (the entries as they stood before the sort)
    for (int64_t i = 0; i < c * K; i++) {
      int32_t unused;
      const size_t o = (size_t)(off * K + i);
      decode_key(hk[(size_t)i], false, &unused, dist_out + o);
      units_out[o] = hu[(size_t)i] < (uint32_t)cb->v.n ? (int32_t)hu[(size_t)i] : -1;
      if (units_out[o] < 0) dist_out[o] = -1.0f;
    }
  }
  return 0;
} ABI_CATCH(somhip_debug_ng_ranks)

extern "C" int somhip_debug_ng_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int K, const double *weights,
                                    int64_t segment, uint32_t *hits, double *sums, double *wsum) try {
  const char *who = "somhip_debug_ng_sums";
  if (!weights || !hits || !sums || !wsum) return fail("%s: null argument", who);
  CHK(ng_check_ranks(K, 1, who));
  CHK(ng_check(cb, ds, first, n, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  segment = ng_segment(K, segment);
  NgBufs b;
  CHK(ng_bind(cb, std::min(n, segment) * K, &b));
  std::vector<double> w(SOMHIP_KNN_MAX, 0.0);
  std::copy(weights, weights + K, w.begin());
  CHK(to_device(e, b.w, w.data(), w.size()));
  CHK(ng_sums_stage(cb, ds, first, n, K, segment, b, nullptr));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  std::vector<double> hs(units * (d + 1));
  CHK(to_host(e, hits, b.hits, units));
  CHK(to_host_sync(e, hs.data(), b.S, hs.size()));
  split_trailing(hs.data(), units, d, sums, wsum);
  return 0;
} ABI_CATCH(somhip_debug_ng_sums)

extern "C" int somhip_debug_ng_update(somhip_codebook *cb, const uint32_t *hits, const double *sums, const double *wsum) try {
  const char *who = "somhip_debug_ng_update";
  CHK(check_codebook(cb, hits && sums && wsum, who));
  CHK(ng_check_codebook(cb, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  NgBufs b;
  CHK(ng_bind(cb, 0, &b));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  std::vector<double> hs(units * (d + 1));
  join_trailing(hs.data(), units, d, sums, wsum);
  CHK(to_device(e, b.S, hs.data(), hs.size()));                        // (hits: what the sums stage returns beside them; W decides, not hits)
  CHK(ng_update_stage(cb, b));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (the host arrays are read until the copies have run)
  return 0;
} ABI_CATCH(somhip_debug_ng_update)

// HIP-event totals of the stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own behind the
// published table): [0] the entries pass per chunk and the grouping, [1] the sums, [2] the update.  The search's launches
// count under their own ids (the published table, somhip_knn_timing).
extern "C" int somhip_ng_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]) try {
  const int kid[3] = {KID_NG_GROUP, KID_NG_SUMS, KID_NG_UPDATE};
  return stage_timing(e, "somhip_ng_timing", kid, 3, launches, total_ms);
} ABI_CATCH(somhip_ng_timing)
