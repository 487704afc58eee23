// host_ngas_dense.inc -- K10d, dense batch neural gas: per epoch the schedule (host, double: a weight for every rank), and per
// chunk of samples the exact distances to every row (K1w's distance stage), the full ranking turned into the chunk's
// weights Q (k_ng_dense_weights), [S | W] = Q^T x [X | 1] on the fp64 MFMA, continued from chunk to chunk (K13's
// k_rslvq_sums); then K10's update; the stages on their own for the tests
// (included by somhip.hip behind host_rslvq.inc: one translation unit, K10's refusals and update, K13's chunk rule, and
// from host_proto.inc the distance and sums stages of a chunk, which K13 runs as well)

static_assert(NGD_MAX == SOMHIP_NG_DENSE_MAX, "the kernel's cap is the header's");

// Step 1 of the definition (include/somhip_ng_dense.h): lambda_t as ng_schedule forms it, and a weight for every rank
static double ngd_lambda(const somhip_ng_params &p, int64_t units, int64_t t) {
  double lambda, w[SOMHIP_KNN_MAX];
  int K;
  ng_schedule(p, units, t, &lambda, &K, w);
  return lambda;
}
static void ngd_weights(double lambda, int64_t units, double *w) {
  for (int64_t r = 0; r < units; r++) w[r] = exp(-(double)r / lambda);
}

// The device arrays of a dense neural-gas call.  SLOT_NGAS: [S | W: units x (dim + 1) doubles] at its start, where K10's
// update reads them; SLOT_NGAS_DENSE: [w: units doubles][d0: n floats]; SLOT_RSLVQ_Q: the chunk's weights Q [chunk][ld],
// ld = 64 * row groups; SLOT_KNN_DIST: the chunk's distances [chunk][ld]; SLOT_SAMPLES: its sample tiles.
struct NgDenseBufs {
  NgBufs ng;
  double *w = nullptr, *Q = nullptr;
  float *d0 = nullptr, *dist = nullptr;
  int64_t chunk = 0, ld = 0;
  int P = 1;                                  // the sort's slots: the smallest power of two >= units
};
static int ngd_bind(somhip_codebook *cb, int64_t n, int64_t chunk, NgDenseBufs *b) {
  somhip_engine *e = cb->e;
  const size_t units = (size_t)cb->v.n;
  CHK(ng_bind(cb, 0, &b->ng));
  void *p;
  CHK(engine_scratch(e, SLOT_NGAS_DENSE, sizeof(double) * units + sizeof(float) * (size_t)n, &p));
  b->w = (double *)p;
  b->d0 = reinterpret_cast<float *>(b->w + units);
  b->ld = cb->v.ngroups * WAVE;
  b->chunk = std::min(chunk, (n + RS_TILE - 1) / RS_TILE * RS_TILE);
  while ((size_t)b->P < units) b->P <<= 1;
  CHK(scratch(e, SLOT_RSLVQ_Q, (size_t)b->chunk * (size_t)b->ld, &b->Q));
  CHK(scratch(e, SLOT_KNN_DIST, (size_t)b->chunk * (size_t)b->ld, &b->dist));
  return 0;
}

// Step 2, b.dist <- every distance of c samples of the run from `off` on, is dist_chunk_stage (host_proto.inc) under
// KID_NG_DENSE_DIST; step 4, [S | W] <- the accumulators continued behind the run's first chunk, is sums_chunk_stage under
// KID_NG_DENSE_SUMS.
// Step 3 for those samples: b.Q <- the chunk's weights, b.d0 at the run's sample numbers (Q null: the ranks stage's outputs
// alone)
static int ngd_weights_stage(somhip_codebook *cb, int64_t off, int64_t c, const NgDenseBufs &b, double *Q, int32_t *rank, float *dunit) {
  return LAUNCH_TIMED(cb->e, KID_NG_DENSE_WEIGHTS, k_ng_dense_weights, dim3((unsigned)c), dim3(NGD_THREADS), sizeof(uint64_t) * (size_t)b.P, cb->v,
                      b.dist, b.ld, off, b.P, b.w, Q, b.d0, rank, dunit);
}
// Steps 2-4 of an epoch with the weights `w` (host, units doubles; read until the copy has run): chunk after chunk.
// q (or null): find_qerror's float chain over the rank-0 distances in data order.
static int ngd_walk(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const double *w, const NgDenseBufs &b, float *q) {
  somhip_engine *e = cb->e;
  CHK(to_device(e, b.w, w, (size_t)cb->v.n));
  for (int64_t off = 0; off < n; off += b.chunk) {
    const int64_t c = std::min(b.chunk, n - off);
    CHK(dist_chunk_stage(cb, ds, first, off, c, KID_NG_DENSE_DIST, b.ld, b.dist));
    CHK(ngd_weights_stage(cb, off, c, b, b.Q, nullptr, nullptr));
    CHK(sums_chunk_stage(cb, ds, first, off, c, KID_NG_DENSE_SUMS, b.Q, b.ld, b.ng.S));
  }
  if (!q) return 0;
  std::vector<float> hd((size_t)n);
  CHK(to_host_sync(e, hd.data(), b.d0, hd.size()));
  float chain = 0.0f;
  for (float d1 : hd) batchmap_q_step(chain, d1);
  *q = chain;
  return 0;
}

// what every dense entry point refuses beyond ng_check
static int ngd_check(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const char *who) {
  CHK(ng_check(cb, ds, first, n, who));
  if (cb->v.n > SOMHIP_NG_DENSE_MAX)
    return fail("%s: %lld rows, more than SOMHIP_NG_DENSE_MAX = %d (a sample's keys sort in one workgroup's LDS)", who, (long long)cb->v.n,
                SOMHIP_NG_DENSE_MAX);
  return 0;
}
static int ngd_check_params(const somhip_ng_params *p, const char *who) {
  if (!p) return fail("%s: null parameters", who);
  if (p->ranks != 0) return fail("%s: ranks %lld: the dense form feeds every rank, ranks must be 0", who, (long long)p->ranks);
  return ng_check_params(p, who);
}

extern "C" int somhip_debug_ng_dense_schedule(const somhip_ng_params *p, int64_t units, int64_t t, double *lambda, double *weights) try {
  const char *who = "somhip_debug_ng_dense_schedule";
  CHK(ngd_check_params(p, who));
  if (!lambda || !weights) return fail("%s: null output", who);
  if (units < 1) return fail("%s: units %lld < 1", who, (long long)units);
  if (t < 0 || t >= p->epochs) return fail("%s: epoch %lld outside [0, %lld)", who, (long long)t, (long long)p->epochs);
  *lambda = ngd_lambda(*p, units, t);
  ngd_weights(*lambda, units, weights);
  return 0;
} ABI_CATCH(somhip_debug_ng_dense_schedule)

extern "C" int somhip_ng_train_dense(somhip_codebook *cb, somhip_dataset *ds, const somhip_ng_params *p, float *qerror_out) try {
  const char *who = "somhip_ng_train_dense";
  if (!cb || !ds) return fail("%s: null handle", who);
  CHK(ngd_check_params(p, who));
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  CHK(ngd_check(cb, ds, p->first, p->n, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  close_accumulations(cb);
  const int64_t units = cb->v.n;
  NgDenseBufs b;
  CHK(ngd_bind(cb, p->n, rslvq_chunk(cb->v.ngroups), &b));
  std::vector<double> w((size_t)units);
  for (int64_t i = 0; i < p->count; i++) {
    float q = 0.0f;
    ngd_weights(ngd_lambda(*p, units, p->start_epoch + i), units, w.data());
    CHK(ngd_walk(cb, ds, p->first, p->n, w.data(), b, qerror_out ? &q : nullptr));
    if (qerror_out) qerror_out[i] = q;
    CHK(ng_update_stage(cb, b.ng));
    HIPCHK(hipStreamSynchronize(e->stream));                            // (w is read until its copy has run, and written for the next epoch)
  }
  return 0;
} ABI_CATCH(somhip_ng_train_dense)

extern "C" int somhip_debug_ng_dense_ranks(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, int32_t *rank_out,
                                           float *dist_out) try {
  const char *who = "somhip_debug_ng_dense_ranks";
  if (!rank_out || !dist_out) return fail("%s: null output", who);
  CHK(ngd_check(cb, ds, first, n, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  NgDenseBufs b;
  CHK(ngd_bind(cb, n, rslvq_chunk(cb->v.ngroups), &b));
  const size_t units = (size_t)cb->v.n, ld = (size_t)b.ld;
  int32_t *rank;
  float *dunit;
  CHK(scratch(e, SLOT_CALL_A, (size_t)b.chunk * ld, &rank));
  CHK(scratch(e, SLOT_CALL_B, (size_t)b.chunk * ld, &dunit));
  std::vector<int32_t> hr((size_t)b.chunk * ld);
  std::vector<float> hd(hr.size());
  for (int64_t off = 0; off < n; off += b.chunk) {
    const int64_t c = std::min(b.chunk, n - off);
    CHK(dist_chunk_stage(cb, ds, first, off, c, KID_NG_DENSE_DIST, b.ld, b.dist));
    CHK(ngd_weights_stage(cb, off, c, b, nullptr, rank, dunit));
    CHK(to_host(e, hr.data(), rank, (size_t)c * ld));
    CHK(to_host_sync(e, hd.data(), dunit, (size_t)c * ld));
    for (size_t i = 0; i < (size_t)c; i++) {
      memcpy(rank_out + ((size_t)off + i) * units, hr.data() + i * ld, sizeof(int32_t) * units);
      memcpy(dist_out + ((size_t)off + i) * units, hd.data() + i * ld, sizeof(float) * units);
    }
  }
  return 0;
} ABI_CATCH(somhip_debug_ng_dense_ranks)

extern "C" int somhip_debug_ng_dense_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, double lambda, int64_t chunk,
                                          double *sums, double *wsum) try {
  const char *who = "somhip_debug_ng_dense_sums";
  if (!sums || !wsum) return fail("%s: null output", who);
  if (!(lambda > 0.0) || std::isinf(lambda)) return fail("%s: lambda %g is not a positive number", who, lambda);
  CHK(ngd_check(cb, ds, first, n, who));
  CHK(rslvq_check_chunk(cb, &chunk, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  NgDenseBufs b;
  CHK(ngd_bind(cb, n, chunk, &b));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  std::vector<double> w(units);
  ngd_weights(lambda, (int64_t)units, w.data());
  CHK(ngd_walk(cb, ds, first, n, w.data(), b, nullptr));
  std::vector<double> hs(units * (d + 1));
  CHK(to_host_sync(e, hs.data(), b.ng.S, hs.size()));
  split_trailing(hs.data(), units, d, sums, wsum);
  return 0;
} ABI_CATCH(somhip_debug_ng_dense_sums)

// HIP-event totals of the stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own behind the
// published table): [0] distances (the sample tiles and k_knn_dist), [1] k_ng_dense_weights, [2] sums
extern "C" int somhip_ng_dense_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]) try {
  const int kid[3] = {KID_NG_DENSE_DIST, KID_NG_DENSE_WEIGHTS, KID_NG_DENSE_SUMS};
  return stage_timing(e, "somhip_ng_dense_timing", kid, 3, launches, total_ms);
} ABI_CATCH(somhip_ng_dense_timing)
