// host_glvq.inc -- K9, batch GLVQ: per epoch the class-wise winners of every sample against the frozen codebook (search),
// the per-sample terms and the grouping by winner of both roles (terms), the per-prototype ordered fp64 sums (sums) and
// the update; the four stages on their own for the tests; the same epoch over data in pieces (somhip_glvq_begin /
// _accumulate / _finish: the sums' chains continued from piece to piece) and over the row blocks of G ranks
// (somhip_glvq_train_ranks)
// (included by somhip.hip behind host_proto.inc and host_batchmap.inc: one translation unit, the trainers' shared checks,
// GlvqBufs, class_scan_walk and copies from host_proto.inc, rocPRIM's sort)

// The route of the search, for every caller: a function of the shape alone.  The list route costs one exact top-8 search
// more than the class-wise scan of its remainder, and the remainder is every sample wherever the eight nearest rows of a
// sample carry one label (measured: all of 100 000 samples at both bench shapes, whose classes are separate clusters with
// 100 rows each).  The shape cannot say how the classes overlap, so the list route is taken where its worst case is cheap:
// where the top-8 search has its two-level pre-filter (512 row groups) and rows are long, it costs 4 % of the class-wise
// scan (100 000 x 1024: 58 of 1451 ms) and can save up to 96 % of it; at 10 000 x 256 it costs 45 % (14 of 31 ms) and the
// class-wise scan runs alone.  Between those two shapes nothing is measured (DESIGN.md K9).
constexpr int64_t GLVQ_LIST_MIN_ROWS = 32768;
constexpr int GLVQ_LIST_MIN_DIM = 512;
constexpr int GLVQ_LIST_WIDTH = 8;              // the entries of a sample's list: the widest exact top-K search
static int glvq_plan(int64_t rows, int dim, int64_t n) {
  return rows >= GLVQ_LIST_MIN_ROWS && dim >= GLVQ_LIST_MIN_DIM && n >= MFMA_MIN_SAMPLES ? SOMHIP_GLVQ_LIST : SOMHIP_GLVQ_DIRECT;
}

// The device arrays of a GLVQ call: GlvqBufs (host_proto.inc), bound here.
// n: the samples of the call, 0 where only the update runs.  state (or null): S and cost are the codebook's own continued
// accumulation, not engine scratch, and the slot holds the rest only (hits is then the piece's own counts).
static int glvq_bind(somhip_codebook *cb, int64_t n, GlvqBufs *b, double *state = nullptr) {
  somhip_engine *e = cb->e;
  const size_t units = (size_t)cb->v.n, ns = (size_t)n, s_len = 2 * units * (size_t)(cb->v.d + 1);
  void *p;
  CHK(engine_scratch(e, SLOT_GLVQ, sizeof(double) * (state ? 0 : s_len + units) + sizeof(uint32_t) * (4 * units + 4), &p));
  b->S = state ? state : (double *)p;
  b->cost = b->S + s_len;
  b->hits = state ? (uint32_t *)p : reinterpret_cast<uint32_t *>(b->cost + units);
  b->starts = b->hits + 2 * units;
  b->correct = b->starts + 2 * (units + 1);
  b->rem_count = b->correct + 1;
  if (n <= 0) return 0;
  for (size_t u = units; u; u >>= 1) b->sort_bits++;
  const hipError_t er = rocprim::radix_sort_pairs(nullptr, b->sort_bytes, b->win, b->win_sorted, b->idx, b->list, ns, 0u, b->sort_bits, e->stream);
  if (er != hipSuccess) return fail("glvq: the sort's size query failed: %s", hipGetErrorString(er));
  const size_t arrays = (sizeof(uint64_t) * 2 * ns + sizeof(double) * 3 * ns + sizeof(uint32_t) * 7 * ns + 255) / 256 * 256;
  CHK(engine_scratch(e, SLOT_GLVQ_LIST, arrays + b->sort_bytes, &p));
  b->keys2 = (uint64_t *)p;
  b->xi = reinterpret_cast<double *>(b->keys2 + 2 * ns);
  b->f = b->xi + 2 * ns;
  b->win = reinterpret_cast<uint32_t *>(b->f + ns);
  b->idx = b->win + 2 * ns;
  b->win_sorted = b->idx + ns;
  b->list = b->win_sorted + ns;
  b->rem = b->list + 2 * ns;
  b->sort_tmp = (char *)p + arrays;
  return 0;
}

// Step 2: b.keys2 <- the two keys of every sample of the run, by the route given.  remainder (or null): the samples the
// class-wise scan took.
static int glvq_search_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int route, const GlvqBufs &b,
                             int64_t *remainder) {
  somhip_engine *e = cb->e;
  if (route == SOMHIP_GLVQ_DIRECT) {
    HIPCHK(hipMemsetAsync(b.keys2, 0xFF, sizeof(uint64_t) * 2 * (size_t)n, e->stream));
    if (remainder) *remainder = n;
    return class_scan_walk(e, cb->v, cb->d_labels, ds, first, n, /*projected*/ nullptr, /*sel*/ nullptr, /*lam*/ nullptr, KID_GLVQ_SEARCH, b.keys2);
  }
  LaunchTimer span(e, KID_GLVQ_SEARCH);
  HIPCHK(hipMemsetAsync(b.rem_count, 0, sizeof(uint32_t), e->stream));
  const int64_t f0 = first % ds->n;
  CHK(knn_chunk_keys(cb, ds, first, n, GLVQ_LIST_WIDTH, 0, [&](int64_t off, int64_t, int64_t c, const uint64_t *dk, int stride) {
    return LAUNCH(e, k_glvq_pick, dim3((unsigned)((c + GLVQ_THREADS - 1) / GLVQ_THREADS)), dim3(GLVQ_THREADS), 0, dk, stride, GLVQ_LIST_WIDTH, off, c,
                  (uint32_t)cb->v.n, cb->d_labels, ds->d_labels, ds->n, f0, b.keys2, b.rem, b.rem_count);
  }));
  uint32_t nrem = 0;
  CHK(to_host_sync(e, &nrem, b.rem_count, 1));      // (the remainder's launches are sized by it)
  if (remainder) *remainder = nrem;
  if (nrem) CHK(class_scan_walk(e, cb->v, cb->d_labels, ds, first, nrem, /*projected*/ nullptr, /*sel*/ b.rem, /*lam*/ nullptr, /*kid*/ -1, b.keys2));
  return 0;
}

// Step 3 and the grouping: the terms, then per role K8's scan of the counts and the stable sort of (winner, sample) by
// winner, which leaves the samples of row u in role r at list[r][starts[r][u] .. starts[r][u + 1]) in data order.
static int glvq_terms_stage(somhip_codebook *cb, int64_t n, float beta, const GlvqBufs &b) {
  somhip_engine *e = cb->e;
  const uint32_t units = (uint32_t)cb->v.n;
  HIPCHK(hipMemsetAsync(b.hits, 0, sizeof(uint32_t) * 2 * (size_t)units, e->stream));
  HIPCHK(hipMemsetAsync(b.correct, 0, sizeof(uint32_t), e->stream));
  CHK(LAUNCH_TIMED(e, KID_GLVQ_TERMS, k_glvq_terms, dim3((unsigned)((n + GLVQ_THREADS - 1) / GLVQ_THREADS)), dim3(GLVQ_THREADS), 0, b.keys2, n, units,
      (double)beta, b.xi, b.f, b.win, b.idx, b.hits, b.correct));
  for (int role = 0; role < 2; role++) {
    CHK(LAUNCH_TIMED(e, KID_GLVQ_TERMS, k_batchmap_starts, dim3(1), dim3(BM_SCAN_THREADS), 0, b.hits + (size_t)role * units, units,
        b.starts + (size_t)role * (units + 1)));
    LaunchTimer t(e, KID_GLVQ_TERMS);                                    // (rocPRIM's own launches, on the engine's stream)
    size_t bytes = b.sort_bytes;
    const hipError_t er = rocprim::radix_sort_pairs(b.sort_tmp, bytes, b.win + (size_t)role * n, b.win_sorted, b.idx, b.list + (size_t)role * n,
                                                    (size_t)n, 0u, b.sort_bits, e->stream);
    if (er != hipSuccess) return fail("glvq: the sort by winner failed: %s", hipGetErrorString(er));
  }
  return 0;
}
// Step 4: b.S and b.cost from the lists.  cont: the chains go on from what b.S and b.cost hold.
static int glvq_sums_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const GlvqBufs &b, bool cont = false) {
  const dim3 grid((unsigned)cb->v.n, (unsigned)((cb->v.d + 2 + BM_SUM_DIMS - 1) / BM_SUM_DIMS), 2);
  if (cont)
    return LAUNCH_TIMED(cb->e, KID_GLVQ_SUMS, k_glvq_sums<true>, grid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->n, ds->d, first % ds->n, n, (uint32_t)cb->v.n,
                        b.list, b.starts, b.xi, b.f, b.S, b.cost);
  return LAUNCH_TIMED(cb->e, KID_GLVQ_SUMS, k_glvq_sums<false>, grid, dim3(BM_SUM_DIMS), 0, ds->d_rows, ds->n, ds->d, first % ds->n, n, (uint32_t)cb->v.n,
                      b.list, b.starts, b.xi, b.f, b.S, b.cost);
}
// Step 5: the rows from b.S and b.hits
static int glvq_update_stage(somhip_codebook *cb, float alpha_t, int64_t n, const GlvqBufs &b) {
  const int64_t threads = cb->v.ngroups * cb->v.d4 * WAVE;
  rows_written(cb);
  return LAUNCH_TIMED(cb->e, KID_GLVQ_UPDATE, k_glvq_update, dim3((unsigned)((threads + GLVQ_THREADS - 1) / GLVQ_THREADS)), dim3(GLVQ_THREADS), 0, cb->v,
                      b.S, b.hits, (double)alpha_t / (double)n);
}

// what every GLVQ entry point refuses before anything is launched
static int glvq_check_codebook(const somhip_codebook *cb, const char *who) {
  if (!cb->d_labels) return fail("%s: the codebook has no labels", who);
  if (is_shard(cb)) return fail("%s: sharded codebook not supported (a shard does not hold the other shards' rows)", who);
  return 0;
}
static int glvq_check(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const char *who) {
  CHK(check_pair(cb, ds, who));
  CHK(glvq_check_codebook(cb, who));
  if (ds->labels.empty()) return fail("%s: the data set has no labels", who);
  if (ds->d_mask) return fail("%s: data with masked components (x) is not supported", who);
  if (first < 0) return fail("%s: first row %lld < 0", who, (long long)first);
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  if (n >= (int64_t)1 << 32) return fail("%s: n %lld does not fit the 32-bit counts", who, (long long)n);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  std::vector<int32_t> cl((size_t)cb->v.n);
  CHK(to_host_sync(e, cl.data(), cb->d_labels, cl.size()));
  std::sort(cl.begin(), cl.end());
  if (cl.front() == cl.back()) return fail("%s: every row of the codebook carries label %d (no other class to be wrong with)", who, (int)cl.front());
  for (int64_t s = 0; s < std::min(n, ds->n); s++) {
    const int32_t l = ds->labels[(size_t)((first + s) % ds->n)];
    if (!std::binary_search(cl.begin(), cl.end(), l))
      return fail("%s: data row %lld carries label %d, which no row of the codebook carries", who, (long long)((first + s) % ds->n), (int)l);
  }
  return dataset_device_labels(ds);
}
static int glvq_check_beta(float beta, const char *who) {
  return beta >= 0.0f ? 0 : fail("%s: sigmoid_beta %g is negative or not a number", who, (double)beta);
}

extern "C" int somhip_debug_glvq_plan(int64_t n_rows, int dim, int64_t n, int32_t *route) try {
  if (!route) return fail("somhip_debug_glvq_plan: null output");
  if (n_rows <= 0 || dim <= 0 || n <= 0) return fail("somhip_debug_glvq_plan: bad shape (%lld x %d, %lld samples)", (long long)n_rows, dim, (long long)n);
  *route = glvq_plan(n_rows, dim, n);
  return 0;
} ABI_CATCH(somhip_debug_glvq_plan)

extern "C" int somhip_glvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_glvq_params *p, double *cost_out,
                                 int64_t *correct_out) try {
  const char *who = "somhip_glvq_train";
  if (!p) return fail("%s: null parameters", who);
  if (!cb || !ds) return fail("%s: null handle", who);
  CHK(check_epochs(p->epochs, who));
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  CHK(check_alpha(p->alpha, who));
  CHK(glvq_check_beta(p->sigmoid_beta, who));
  CHK(glvq_check(cb, ds, p->first, p->n, who));
  somhip_engine *e = cb->e;
  GlvqBufs b;
  CHK(glvq_bind(cb, p->n, &b));
  const int route = glvq_plan(cb->v.n, cb->v.d, p->n);
  std::vector<double> hc((size_t)(cost_out ? cb->v.n : 0));
  for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
    const float alpha_t = linear_rate(p->alpha, p->epochs, t);
    CHK(glvq_search_stage(cb, ds, p->first, p->n, route, b, nullptr));
    CHK(glvq_terms_stage(cb, p->n, p->sigmoid_beta, b));
    CHK(glvq_sums_stage(cb, ds, p->first, p->n, b));
    if (cost_out || correct_out) {
      uint32_t correct = 0;
      if (cost_out) CHK(to_host(e, hc.data(), b.cost, hc.size()));
      CHK(to_host_sync(e, &correct, b.correct, 1));
      if (cost_out) cost_out[t - p->start_epoch] = cost_figure(hc, (double)p->n);
      if (correct_out) correct_out[t - p->start_epoch] = (int64_t)correct;
    }
    CHK(glvq_update_stage(cb, alpha_t, p->n, b));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_glvq_train)

extern "C" int somhip_debug_glvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int route, float *dplus,
                                        int32_t *iplus, float *dminus, int32_t *iminus, int64_t *remainder) try {
  const char *who = "somhip_debug_glvq_search";
  if (!dplus || !iplus || !dminus || !iminus) return fail("%s: null output", who);
  if (route != SOMHIP_GLVQ_PLAN && route != SOMHIP_GLVQ_DIRECT && route != SOMHIP_GLVQ_LIST) return fail("%s: unknown route %d", who, route);
  CHK(glvq_check(cb, ds, first, n, who));
  somhip_engine *e = cb->e;
  GlvqBufs b;
  CHK(glvq_bind(cb, n, &b));
  CHK(glvq_search_stage(cb, ds, first, n, route == SOMHIP_GLVQ_PLAN ? glvq_plan(cb->v.n, cb->v.d, n) : route, b, remainder));
  return glvq_keys_to_host(e, b, n, dplus, iplus, dminus, iminus);
} ABI_CATCH(somhip_debug_glvq_search)

extern "C" int somhip_debug_glvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta,
                                      double *xi_plus, double *xi_minus, double *f, double *sums_plus, uint32_t *n_plus,
                                      double *sums_minus, uint32_t *n_minus, double *cost, int64_t *correct) try {
  const char *who = "somhip_debug_glvq_sums";
  if (!xi_plus || !xi_minus || !f || !sums_plus || !n_plus || !sums_minus || !n_minus || !cost || !correct) return fail("%s: null output", who);
  CHK(glvq_check_beta(sigmoid_beta, who));
  CHK(glvq_check(cb, ds, first, n, who));
  somhip_engine *e = cb->e;
  GlvqBufs b;
  CHK(glvq_bind(cb, n, &b));
  CHK(glvq_search_stage(cb, ds, first, n, glvq_plan(cb->v.n, cb->v.d, n), b, nullptr));
  CHK(glvq_terms_stage(cb, n, sigmoid_beta, b));
  CHK(glvq_sums_stage(cb, ds, first, n, b));
  uint32_t hcorrect = 0;
  CHK(glvq_sums_to_host(cb, b, n, xi_plus, xi_minus, f, sums_plus, n_plus, sums_minus, n_minus, cost));
  CHK(to_host_sync(e, &hcorrect, b.correct, 1));
  *correct = (int64_t)hcorrect;
  return 0;
} ABI_CATCH(somhip_debug_glvq_sums)

extern "C" int somhip_debug_glvq_update(somhip_codebook *cb, float alpha_t, int64_t n, const double *sums_plus, const uint32_t *n_plus,
                                        const double *sums_minus, const uint32_t *n_minus) try {
  const char *who = "somhip_debug_glvq_update";
  CHK(check_codebook(cb, sums_plus && n_plus && sums_minus && n_minus, who));
  CHK(glvq_check_codebook(cb, who));
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  GlvqBufs b;
  CHK(glvq_bind(cb, 0, &b));
  CHK(glvq_sums_to_device(cb, b, sums_plus, n_plus, sums_minus, n_minus));
  CHK(glvq_update_stage(cb, alpha_t, n, b));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (the host arrays are read until the copies have run)
  return 0;
} ABI_CATCH(somhip_debug_glvq_update)

// HIP-event totals of the stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own behind the
// published table): [0] search, [1] terms and grouping, [2] sums, [3] update
extern "C" int somhip_glvq_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]) try {
  const int kid[4] = {KID_GLVQ_SEARCH, KID_GLVQ_TERMS, KID_GLVQ_SUMS, KID_GLVQ_UPDATE};
  return stage_timing(e, "somhip_glvq_timing", kid, 4, launches, total_ms);
} ABI_CATCH(somhip_glvq_timing)

// ---------------------------------------------------------------------------------
// The epoch over data in pieces (include/somhip_glvq_pieces.h).  The state is one device blob the codebook owns:
// [Sp | sp][Sm | sm] as 2 x rows x (dim + 1) doubles, cost[rows] doubles, np[rows] and nm[rows] as uint32, then the tail --
// the samples taken and the correct ones among them.  Nothing of an accumulation lives on the host between calls, so the
// blob copied into another codebook of the same shape (its own state opened by _begin) continues there: that is what hands
// the chains from rank to rank.
// ---------------------------------------------------------------------------------
struct GlvqTail { uint64_t samples, correct; };
static_assert(sizeof(GlvqTail) == 16, "the tail of the GLVQ state is two words of 8 bytes");
static size_t glvq_state_doubles(const somhip_codebook *cb) { return (size_t)cb->v.n * (2 * (size_t)(cb->v.d + 1) + 1); }
static size_t glvq_state_bytes(const somhip_codebook *cb) {
  return sizeof(double) * glvq_state_doubles(cb) + sizeof(uint32_t) * 2 * (size_t)cb->v.n + sizeof(GlvqTail);
}
static uint32_t *glvq_state_counts(const somhip_codebook *cb) { return reinterpret_cast<uint32_t *>(cb->gl_state + glvq_state_doubles(cb)); }
static GlvqTail *glvq_state_tail(const somhip_codebook *cb) { return reinterpret_cast<GlvqTail *>(glvq_state_counts(cb) + 2 * (size_t)cb->v.n); }

// opens the state as all-zero bits (+0.0 throughout, counts and tail 0)
static int glvq_state_open(somhip_codebook *cb) {
  if (!cb->gl_state) HIPCHK(hipMalloc((void **)&cb->gl_state, glvq_state_bytes(cb)));
  HIPCHK(hipMemsetAsync(cb->gl_state, 0, glvq_state_bytes(cb), cb->e->stream));
  cb->gl_open = true;
  cb->gl_moved = false;
  return 0;
}
static void glvq_state_free(somhip_codebook *cb) {
  if (cb->gl_state) (void)hipFree(cb->gl_state);
  cb->gl_state = nullptr;
  cb->gl_open = cb->gl_moved = false;
}
static int glvq_check_open(const somhip_codebook *cb, const char *who) {
  return cb->gl_open && cb->gl_state ? 0 : fail("%s: no accumulation is open on this codebook (somhip_glvq_begin first; a call that writes "
                                                 "the rows closes it)", who);
}
// The tail as the pieces so far left it, and the refusal of a piece of n samples that would take the total to 2^32: a copy
// and a comparison, before anything is bound or launched.
static int glvq_read_tail(somhip_codebook *cb, int64_t n, const char *who, GlvqTail *tail) {
  CHK(to_host_sync(cb->e, tail, glvq_state_tail(cb), 1));
  if (tail->samples + (uint64_t)n >= (uint64_t)1 << 32)
    return fail("%s: %llu + %lld samples do not fit the 32-bit counts", who, (unsigned long long)tail->samples, (long long)n);
  return 0;
}
// The sums half of a piece whose search, terms and grouping have run into b (bound with the state): the chains go on, the
// counts and the tail grow -- on the device, by one writer per word.
static int glvq_take_piece(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const GlvqBufs &b) {
  const uint32_t words = 2 * (uint32_t)cb->v.n;
  CHK(glvq_sums_stage(cb, ds, first, n, b, true));
  return LAUNCH_TIMED(cb->e, KID_GLVQ_SUMS, k_glvq_counts, dim3((words + GLVQ_THREADS - 1) / GLVQ_THREADS), dim3(GLVQ_THREADS), 0, b.hits, b.correct,
                      (uint64_t)n, words, glvq_state_counts(cb), reinterpret_cast<uint64_t *>(glvq_state_tail(cb)));
}
// Step 5 from the state, whose tail the caller has read (samples > 0), with the epoch's two figures: the host's chain over
// cost[] in row order / samples, and the tail's count.  The state stays open, moved.
static int glvq_finish_state(somhip_codebook *cb, float alpha_t, const GlvqTail &tail, double *cost_out, int64_t *correct_out) {
  somhip_engine *e = cb->e;
  GlvqBufs b;
  b.S = cb->gl_state;
  b.cost = b.S + 2 * (size_t)cb->v.n * (size_t)(cb->v.d + 1);
  b.hits = glvq_state_counts(cb);
  if (cost_out) {
    std::vector<double> hc((size_t)cb->v.n);
    CHK(to_host_sync(e, hc.data(), b.cost, hc.size()));
    *cost_out = cost_figure(hc, (double)tail.samples);
  }
  if (correct_out) *correct_out = (int64_t)tail.correct;
  CHK(glvq_update_stage(cb, alpha_t, (int64_t)tail.samples, b));
  cb->gl_open = cb->gl_moved = true;                                    // (the update closes every accumulation; this one stays, moved)
  return 0;
}

extern "C" int somhip_glvq_begin(somhip_codebook *cb) try {
  const char *who = "somhip_glvq_begin";
  CHK(check_codebook(cb, true, who));
  CHK(glvq_check_codebook(cb, who));
  HIPCHK(hipSetDevice(cb->e->device));
  CHK(glvq_state_open(cb));
  HIPCHK(hipStreamSynchronize(cb->e->stream));
  return 0;
} ABI_CATCH(somhip_glvq_begin)

extern "C" int somhip_glvq_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta) try {
  const char *who = "somhip_glvq_accumulate";
  CHK(check_pair(cb, ds, who));
  CHK(glvq_check_beta(sigmoid_beta, who));
  CHK(glvq_check(cb, ds, first, n, who));
  CHK(glvq_check_open(cb, who));
  if (cb->gl_moved) return fail("%s: the codebook has moved (somhip_glvq_finish has run; somhip_glvq_begin opens the next epoch)", who);
  somhip_engine *e = cb->e;
  GlvqTail tail;
  CHK(glvq_read_tail(cb, n, who, &tail));                               // (the last refusal: nothing is bound before it)
  GlvqBufs b;
  CHK(glvq_bind(cb, n, &b, cb->gl_state));
  CHK(glvq_search_stage(cb, ds, first, n, glvq_plan(cb->v.n, cb->v.d, n), b, nullptr));
  CHK(glvq_terms_stage(cb, n, sigmoid_beta, b));
  CHK(glvq_take_piece(cb, ds, first, n, b));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_glvq_accumulate)

extern "C" int somhip_glvq_finish(somhip_codebook *cb, float alpha_t, double *cost_out, int64_t *correct_out, int64_t *samples_out) try {
  const char *who = "somhip_glvq_finish";
  CHK(check_codebook(cb, true, who));
  CHK(glvq_check_codebook(cb, who));
  CHK(glvq_check_open(cb, who));
  if (!(alpha_t >= 0.0f)) return fail("%s: alpha_t %g is negative or not a number", who, (double)alpha_t);
  if (cb->gl_moved) return fail("%s: the codebook has moved (somhip_glvq_finish has run; somhip_glvq_begin opens the next epoch)", who);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  GlvqTail tail;
  CHK(glvq_read_tail(cb, 0, who, &tail));
  if (tail.samples == 0) return fail("%s: the state holds no sample", who);
  CHK(glvq_finish_state(cb, alpha_t, tail, cost_out, correct_out));
  if (samples_out) *samples_out = (int64_t)tail.samples;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_glvq_finish)

extern "C" int somhip_glvq_end(somhip_codebook *cb) try {
  CHK(check_codebook(cb, true, "somhip_glvq_end"));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  glvq_state_free(cb);
  return 0;
} ABI_CATCH(somhip_glvq_end)

extern "C" int somhip_glvq_state(somhip_codebook *cb, void **dev_state, int64_t *bytes) try {
  CHK(check_codebook(cb, dev_state && bytes, "somhip_glvq_state"));
  CHK(glvq_check_open(cb, "somhip_glvq_state"));
  *dev_state = cb->gl_state;
  *bytes = (int64_t)glvq_state_bytes(cb);
  return 0;
} ABI_CATCH(somhip_glvq_state)

// The epochs of somhip_glvq_train over the row blocks of the communicator's ranks, block by block in rank order.  Every
// rank holds the whole codebook.  Per epoch: search, terms and grouping on every rank's own block at once; then, rank after
// rank, the continued sums on the rank whose turn it is and the state broadcast from it; then the same update from the
// same state on every rank.
extern "C" int somhip_glvq_train_ranks(somhip_codebook *cb, somhip_dataset *block, const somhip_glvq_params *p, somhip_comm *c,
                                       double *cost_out, int64_t *correct_out) try {
  const char *who = "somhip_glvq_train_ranks";
  CHK(check_codebook(cb, p && c, who));
  const bool empty = p->n == 0;                                          // a rank whose block holds no row: legal here and only here
  CHK(check_epochs(p->epochs, who));
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  CHK(check_alpha(p->alpha, who));
  CHK(glvq_check_beta(p->sigmoid_beta, who));
  if (c->e != cb->e) return fail("%s: codebook and communicator belong to different engines", who);
  if (empty) CHK(glvq_check_codebook(cb, who));
  else CHK(glvq_check(cb, block, p->first, p->n, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  // The blocks' rows together must fit the 32-bit counts: every rank learns the total (summed as two 16-bit halves, so the
  // words cannot overflow) and refuses alike, before any rank has launched anything.
  struct Words {
    uint32_t *d = nullptr;
    ~Words() { if (d) (void)hipFree(d); }
  } w;
  HIPCHK(hipMalloc((void **)&w.d, 2 * sizeof(uint32_t)));
  uint32_t halves[2] = {(uint32_t)(p->n >> 16), (uint32_t)(p->n & 0xffff)};
  CHK(to_device(e, w.d, halves, 2));
  HIPCHK(hipStreamSynchronize(e->stream));
  CHK(somhip_comm_allreduce_sum_u32(c, w.d, 2));
  CHK(to_host_sync(e, halves, w.d, 2));
  const uint64_t total = ((uint64_t)halves[0] << 16) + halves[1];
  if (total >= (uint64_t)1 << 32) return fail("%s: the ranks' %llu samples do not fit the 32-bit counts", who, (unsigned long long)total);
  if (total == 0) return fail("%s: no rank holds a row", who);
  auto epochs = [&]() -> int {
    const int route = empty ? SOMHIP_GLVQ_DIRECT : glvq_plan(cb->v.n, cb->v.d, p->n);
    CHK(glvq_state_open(cb));                                           // (the blob exists from here on: its address is bound once;
    GlvqBufs b;                                                         //  every epoch opens it again, which re-zeroes it)
    CHK(glvq_bind(cb, p->n, &b, cb->gl_state));
    for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
      const float alpha_t = linear_rate(p->alpha, p->epochs, t);
      CHK(glvq_state_open(cb));
      if (!empty) {
        CHK(glvq_search_stage(cb, block, p->first, p->n, route, b, nullptr));
        CHK(glvq_terms_stage(cb, p->n, p->sigmoid_beta, b));
      }
      for (int root = 0; root < c->world; root++) {
        if (root == c->rank && !empty) CHK(glvq_take_piece(cb, block, p->first, p->n, b));
        HIPCHK(hipStreamSynchronize(e->stream));
        CHK(somhip_comm_broadcast(c, cb->gl_state, (int64_t)glvq_state_bytes(cb), root));
      }
      GlvqTail tail;
      CHK(to_host_sync(e, &tail, glvq_state_tail(cb), 1));
      if (tail.samples != total) return fail("%s: the state holds %llu of %llu samples", who, (unsigned long long)tail.samples, (unsigned long long)total);
      CHK(glvq_finish_state(cb, alpha_t, tail, cost_out ? cost_out + (t - p->start_epoch) : nullptr,
                            correct_out ? correct_out + (t - p->start_epoch) : nullptr));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
  };
  const int rc = epochs();
  // The state was the epochs' own, on every way out: closed, so that no later _finish updates from a state that was
  // broadcast half way, and freed.
  (void)hipStreamSynchronize(e->stream);
  glvq_state_free(cb);
  return rc;
} ABI_CATCH(somhip_glvq_train_ranks)
