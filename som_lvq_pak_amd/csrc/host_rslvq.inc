// host_rslvq.inc -- K13, batch Robust Soft LVQ: per epoch and chunk of samples the exact distances to every row (K1w's
// distance stage), the posteriors and their coefficients Q (posterior), [G | c] = Q^T x [X | 1] on the fp64 MFMA, continued
// from chunk to chunk (sums); then the update; the stages on their own for the tests
// (included by somhip.hip behind host_gmlvq.inc: one translation unit, K9's refusals, and from host_proto.inc the distance
// and sums stages of a chunk, which the dense neural gas runs as well)

constexpr int64_t RSLVQ_CHUNK_MAX = 4096;                       // samples of a chunk at most
constexpr size_t RSLVQ_Q_BYTES = (size_t)256 << 20;             // ... and the room its Q may take
// The chunk of the training and of the public evaluation, for every caller: a function of the codebook's rows alone.
// min(4096, the largest multiple of 64 whose Q chunk [chunk][64 * row groups] of doubles stays within 256 MiB), 64 at least.
static int64_t rslvq_chunk(int64_t ngroups) {
  const int64_t fit = (int64_t)(RSLVQ_Q_BYTES / (sizeof(double) * (size_t)ngroups * WAVE)) / RS_TILE * RS_TILE;
  return std::max<int64_t>(RS_TILE, std::min(RSLVQ_CHUNK_MAX, fit));
}

// The device arrays of an RSLVQ call.  SLOT_RSLVQ: [G | c: rows x (dim + 1) doubles][cost_s: n][pown: n][correct_s: n];
// SLOT_RSLVQ_Q: the Q chunk [chunk][ld], ld = 64 * row groups; SLOT_KNN_DIST: the chunk's distances [chunk][ld];
// SLOT_SAMPLES: its sample tiles.
struct RslvqBufs {
  double *G = nullptr, *cost_s = nullptr, *pown = nullptr, *Q = nullptr;
  int32_t *correct_s = nullptr;
  float *dist = nullptr;
  int64_t chunk = 0, ld = 0;
};
// n: the samples of the call, 0 where only the update runs; chunk: 0 where no chunk is walked
static int rslvq_bind(somhip_codebook *cb, int64_t n, int64_t chunk, RslvqBufs *b) {
  somhip_engine *e = cb->e;
  const size_t g_len = (size_t)cb->v.n * (size_t)(cb->v.d + 1), ns = (size_t)n;
  void *p;
  CHK(engine_scratch(e, SLOT_RSLVQ, sizeof(double) * (g_len + 2 * ns) + sizeof(int32_t) * ns, &p));
  b->G = (double *)p;
  b->cost_s = b->G + g_len;
  b->pown = b->cost_s + ns;
  b->correct_s = reinterpret_cast<int32_t *>(b->pown + ns);
  b->ld = cb->v.ngroups * WAVE;
  b->chunk = std::min(chunk, (n + RS_TILE - 1) / RS_TILE * RS_TILE);
  if (chunk <= 0) return 0;
  CHK(scratch(e, SLOT_RSLVQ_Q, (size_t)b->chunk * (size_t)b->ld, &b->Q));
  CHK(scratch(e, SLOT_KNN_DIST, (size_t)b->chunk * (size_t)b->ld, &b->dist));
  return 0;
}

// Step 2, b.dist <- every distance of c samples of the run from `off` on, is dist_chunk_stage (host_proto.inc) under
// KID_RSLVQ_DIST; step 4, b.G <- the chains continued behind the run's first chunk, is sums_chunk_stage under KID_RSLVQ_SUMS.
// Step 3 for those samples: b.Q <- the chunk's coefficients; cost_s, pown, correct_s at the run's sample numbers
static int rslvq_posterior_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t off, int64_t c, float sigma2,
                                 const RslvqBufs &b) {
  return LAUNCH_TIMED(cb->e, KID_RSLVQ_POSTERIOR, k_rslvq_posterior, dim3((unsigned)((c + RS_WAVES - 1) / RS_WAVES)), dim3(RS_WAVES * WAVE), 0,
                      cb->v, b.dist, b.ld, c, off, cb->d_labels, ds->d_labels, ds->n, first % ds->n, 2.0 * (double)sigma2, b.Q, b.cost_s,
                      b.correct_s, b.pown);
}
// Step 5: the rows from b.G
static int rslvq_update_stage(somhip_codebook *cb, float alpha_t, float sigma2, int64_t n, const RslvqBufs &b) {
  const int64_t threads = cb->v.ngroups * cb->v.d4 * WAVE;
  rows_written(cb);
  const double den = (double)sigma2 * (double)n;
  return LAUNCH_TIMED(cb->e, KID_RSLVQ_UPDATE, k_rslvq_update, dim3((unsigned)((threads + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, cb->v,
                      b.G, (double)alpha_t / den);
}
// Steps 2 and 3 (and 4 with sums) over the whole run, chunk after chunk
static int rslvq_walk(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigma2, bool sums, const RslvqBufs &b) {
  for (int64_t off = 0; off < n; off += b.chunk) {
    const int64_t c = std::min(b.chunk, n - off);
    CHK(dist_chunk_stage(cb, ds, first, off, c, KID_RSLVQ_DIST, b.ld, b.dist));
    CHK(rslvq_posterior_stage(cb, ds, first, off, c, sigma2, b));
    if (sums) CHK(sums_chunk_stage(cb, ds, first, off, c, KID_RSLVQ_SUMS, b.Q, b.ld, b.G));
  }
  return 0;
}
// cost (or null) <- the host's fp64 chain over cost_s in data order / n; correct (or null) <- the count
static int rslvq_figures(somhip_codebook *cb, int64_t n, const RslvqBufs &b, double *cost, int64_t *correct) {
  somhip_engine *e = cb->e;
  std::vector<double> hc((size_t)(cost ? n : 0));
  std::vector<int32_t> hr((size_t)(correct ? n : 0));
  if (cost) CHK(to_host(e, hc.data(), b.cost_s, hc.size()));
  if (correct) CHK(to_host(e, hr.data(), b.correct_s, hr.size()));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (cost) *cost = cost_figure(hc, (double)n);
  if (correct) {
    int64_t right = 0;
    for (int32_t r : hr) right += r;
    *correct = right;
  }
  return 0;
}

static int rslvq_check_sigma2(float sigma2, const char *who) {
  return std::isfinite(sigma2) && sigma2 > 0.0f ? 0 : fail("%s: sigma2 %g is not a finite number above 0", who, (double)sigma2);
}
// a debug entry's chunk: 0 is the rule's; else a multiple of 64 up to 4096 that the rule's room holds
static int rslvq_check_chunk(const somhip_codebook *cb, int64_t *chunk, const char *who) {
  const int64_t rule = rslvq_chunk(cb->v.ngroups);
  if (*chunk == 0) *chunk = rule;
  if (*chunk < RS_TILE || *chunk % RS_TILE || *chunk > RSLVQ_CHUNK_MAX)
    return fail("%s: chunk %lld is not a multiple of %d in [%d, %lld]", who, (long long)*chunk, RS_TILE, RS_TILE, (long long)RSLVQ_CHUNK_MAX);
  *chunk = std::min(*chunk, rule);
  return 0;
}

extern "C" int somhip_rslvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_rslvq_params *p, double *cost_out,
                                  int64_t *correct_out) try {
  const char *who = "somhip_rslvq_train";
  if (!p) return fail("%s: null parameters", who);
  if (!cb || !ds) return fail("%s: null handle", who);
  CHK(check_epochs(p->epochs, who));
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  CHK(check_alpha(p->alpha, who));
  CHK(rslvq_check_sigma2(p->sigma2, who));
  CHK(glvq_check(cb, ds, p->first, p->n, who));
  somhip_engine *e = cb->e;
  RslvqBufs b;
  CHK(rslvq_bind(cb, p->n, rslvq_chunk(cb->v.ngroups), &b));
  for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
    const float alpha_t = linear_rate(p->alpha, p->epochs, t);
    CHK(rslvq_walk(cb, ds, p->first, p->n, p->sigma2, true, b));
    if (cost_out || correct_out)
      CHK(rslvq_figures(cb, p->n, b, cost_out ? cost_out + (t - p->start_epoch) : nullptr, correct_out ? correct_out + (t - p->start_epoch) : nullptr));
    CHK(rslvq_update_stage(cb, alpha_t, p->sigma2, p->n, b));
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_rslvq_train)

extern "C" int somhip_rslvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigma2, double *cost,
                                   int64_t *correct, double *pown) try {
  const char *who = "somhip_rslvq_search";
  if (!cost || !correct) return fail("%s: null output", who);
  CHK(rslvq_check_sigma2(sigma2, who));
  CHK(glvq_check(cb, ds, first, n, who));
  RslvqBufs b;
  CHK(rslvq_bind(cb, n, rslvq_chunk(cb->v.ngroups), &b));
  CHK(rslvq_walk(cb, ds, first, n, sigma2, false, b));
  if (pown) CHK(to_host(cb->e, pown, b.pown, (size_t)n));
  return rslvq_figures(cb, n, b, cost, correct);
} ABI_CATCH(somhip_rslvq_search)

extern "C" int somhip_debug_rslvq_chunk(int64_t n_rows, int64_t *chunk, int64_t *ld) try {
  if (!chunk || !ld) return fail("somhip_debug_rslvq_chunk: null output");
  if (n_rows <= 0) return fail("somhip_debug_rslvq_chunk: %lld rows", (long long)n_rows);
  const int64_t ngroups = (n_rows + WAVE - 1) / WAVE;
  *chunk = rslvq_chunk(ngroups);
  *ld = ngroups * WAVE;
  return 0;
} ABI_CATCH(somhip_debug_rslvq_chunk)

extern "C" int somhip_debug_rslvq_posterior(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigma2, int64_t chunk,
                                            double *q_out, double *cost_s, int32_t *correct_s, double *pown) try {
  const char *who = "somhip_debug_rslvq_posterior";
  if (!q_out || !cost_s || !correct_s || !pown) return fail("%s: null output", who);
  CHK(rslvq_check_sigma2(sigma2, who));
  CHK(glvq_check(cb, ds, first, n, who));
  CHK(rslvq_check_chunk(cb, &chunk, who));
  somhip_engine *e = cb->e;
  RslvqBufs b;
  CHK(rslvq_bind(cb, n, chunk, &b));
  for (int64_t off = 0; off < n; off += b.chunk) {
    const int64_t c = std::min(b.chunk, n - off);
    CHK(dist_chunk_stage(cb, ds, first, off, c, KID_RSLVQ_DIST, b.ld, b.dist));
    CHK(rslvq_posterior_stage(cb, ds, first, off, c, sigma2, b));
    CHK(to_host_sync(e, q_out + (size_t)off * (size_t)b.ld, b.Q, (size_t)c * (size_t)b.ld));
  }
  CHK(to_host(e, cost_s, b.cost_s, (size_t)n));
  CHK(to_host(e, pown, b.pown, (size_t)n));
  CHK(to_host_sync(e, correct_s, b.correct_s, (size_t)n));
  return 0;
} ABI_CATCH(somhip_debug_rslvq_posterior)

extern "C" int somhip_debug_rslvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int64_t chunk, const double *q_in,
                                       double *G, double *c_out) try {
  const char *who = "somhip_debug_rslvq_sums";
  if (!q_in || !G || !c_out) return fail("%s: null argument", who);
  CHK(glvq_check(cb, ds, first, n, who));
  CHK(rslvq_check_chunk(cb, &chunk, who));
  somhip_engine *e = cb->e;
  RslvqBufs b;
  CHK(rslvq_bind(cb, n, chunk, &b));
  for (int64_t off = 0; off < n; off += b.chunk) {
    const int64_t c = std::min(b.chunk, n - off);
    CHK(to_device(e, b.Q, q_in + (size_t)off * (size_t)b.ld, (size_t)c * (size_t)b.ld));
    CHK(sums_chunk_stage(cb, ds, first, off, c, KID_RSLVQ_SUMS, b.Q, b.ld, b.G));
    HIPCHK(hipStreamSynchronize(e->stream));                            // (the host array is read until the copy has run)
  }
  const size_t units = (size_t)cb->v.n, ldg = (size_t)cb->v.d + 1;
  std::vector<double> hg(units * ldg);
  CHK(to_host_sync(e, hg.data(), b.G, hg.size()));
  split_trailing(hg.data(), units, ldg - 1, G, c_out);
  return 0;
} ABI_CATCH(somhip_debug_rslvq_sums)

extern "C" int somhip_debug_rslvq_update(somhip_codebook *cb, float alpha_t, float sigma2, int64_t n, const double *G, const double *c_in) try {
  const char *who = "somhip_debug_rslvq_update";
  CHK(check_codebook(cb, G && c_in, who));
  CHK(glvq_check_codebook(cb, who));
  CHK(rslvq_check_sigma2(sigma2, who));
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  RslvqBufs b;
  CHK(rslvq_bind(cb, 0, 0, &b));
  const size_t units = (size_t)cb->v.n, ldg = (size_t)cb->v.d + 1;
  std::vector<double> hg(units * ldg);
  join_trailing(hg.data(), units, ldg - 1, G, c_in);
  CHK(to_device(e, b.G, hg.data(), hg.size()));
  CHK(rslvq_update_stage(cb, alpha_t, sigma2, n, b));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (the host array is read until the copy has run)
  return 0;
} ABI_CATCH(somhip_debug_rslvq_update)

// HIP-event totals of the stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own behind the
// published table): [0] distances (the sample tiles and k_knn_dist), [1] posteriors, [2] sums, [3] update
extern "C" int somhip_rslvq_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]) try {
  const int kid[4] = {KID_RSLVQ_DIST, KID_RSLVQ_POSTERIOR, KID_RSLVQ_SUMS, KID_RSLVQ_UPDATE};
  return stage_timing(e, "somhip_rslvq_timing", kid, 4, launches, total_ms);
} ABI_CATCH(somhip_rslvq_timing)
