// host_gmlvq.inc -- K12, batch GMLVQ: K9's epoch under d(x, w) = |Omega (x - w)|^2 -- the fp64 projection of the samples and
// the rows, K9's class-wise scan on the projected tiles, K9's terms, grouping and sums (unchanged), the block-wise ordered
// gradient of Omega with its reduction, the update through Omega^T Omega, and Omega's step on the host; the stages on their
// own for the tests
// (included by somhip.hip behind host_grlvq.inc: one translation unit; K9's checks, binding, terms and sums stages by name,
// K11's check of eps, and the trainers' shared pieces of host_proto.inc: the class-wise scan's walk over tiles that are
// there already, the family's copies)

// The device arrays of a GMLVQ call beside K9's (GlvqBufs: SLOT_GLVQ, SLOT_GLVQ_LIST).  SLOT_GMLVQ: [vt: the projected storage
// tiles, groups x d4m x 64 float4][xt: the projected sample tiles of the whole run, ceil(n / 32) x d4m x 32 float4]
// [g: rows x dim doubles][P: rows x m doubles][Gm: m x dim doubles][om: m x dim floats][omT: dim x m floats].
// SLOT_GMLVQ_PART: [blocks of GMLVQ_BLOCK samples][m][dim] doubles (100 000 samples x 1024 x rank 1024: 25 x 8 MiB = 210 MB).
struct GmlvqBufs {
  GlvqBufs g;
  CbView pv{};                                   // the codebook's view over vt: d = m, d4 = d4m, everything else the codebook's
  int m = 0, d4m = 0;
  int64_t nblocks = 0;
  float *vt = nullptr, *xt = nullptr, *om = nullptr, *omT = nullptr;
  double *gbuf = nullptr, *P = nullptr, *Gm = nullptr, *part = nullptr;
};
// n: the samples of the call, 0 where only the update runs
static int gmlvq_bind(somhip_codebook *cb, int64_t n, int m, GmlvqBufs *b) {
  if ((n + GMLVQ_BLOCK - 1) / GMLVQ_BLOCK > 65535) return fail("gmlvq: %lld samples are more than 65535 blocks of %d", (long long)n, GMLVQ_BLOCK);
  CHK(glvq_bind(cb, n, &b->g));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d, mm = (size_t)m, d4m = (mm + 3) / 4;
  const size_t vt_len = (size_t)cb->v.ngroups * d4m * WAVE * 4, xt_len = ((size_t)n + GLVQ_S - 1) / GLVQ_S * d4m * GLVQ_S * 4;
  void *p;
  CHK(engine_scratch(cb->e, SLOT_GMLVQ, sizeof(float) * (vt_len + xt_len + 2 * mm * d) + sizeof(double) * (units * d + units * mm + mm * d), &p));
  b->m = m;
  b->d4m = (int)d4m;
  b->vt = (float *)p;                            // (first: 16-byte aligned, and whole float4 in length, as xt)
  b->xt = b->vt + vt_len;
  b->gbuf = reinterpret_cast<double *>(b->xt + xt_len);
  b->P = b->gbuf + units * d;
  b->Gm = b->P + units * mm;
  b->om = reinterpret_cast<float *>(b->Gm + mm * d);
  b->omT = b->om + mm * d;
  b->pv = cb->v;
  b->pv.tiles = b->vt;
  b->pv.d = m;
  b->pv.d4 = (int)d4m;
  b->nblocks = (n + GMLVQ_BLOCK - 1) / GMLVQ_BLOCK;
  if (n > 0) CHK(scratch(cb->e, SLOT_GMLVQ_PART, (size_t)b->nblocks * mm * d, &b->part));
  return 0;
}

// what every entry point asks of the rank and of Omega before anything is launched
static int gmlvq_check_omega(const float *omega, int rank, int d, bool nonzero, const char *who) {
  if (rank < 1 || rank > d) return fail("%s: rank %d outside [1, %d]", who, rank, d);
  if (!omega) return fail("%s: null omega", who);
  bool any = false;
  for (size_t i = 0; i < (size_t)rank * d; i++) {
    if (!std::isfinite(omega[i])) return fail("%s: omega[%d][%d] = %g is not a finite number", who, (int)(i / d), (int)(i % d), (double)omega[i]);
    any = any || omega[i] != 0.0f;
  }
  if (nonzero && !any) return fail("%s: omega is all zero (every distance would be 0)", who);
  return 0;
}

// omega -> b.om and b.omT through `stage` (2 m dim floats the caller keeps until the stream has been waited for)
static int gmlvq_put_omega(somhip_codebook *cb, const float *omega, std::vector<float> &stage, const GmlvqBufs &b) {
  const size_t d = (size_t)cb->v.d, m = (size_t)b.m;
  stage.resize(2 * m * d);
  std::copy(omega, omega + m * d, stage.begin());
  for (size_t r = 0; r < m; r++)
    for (size_t k = 0; k < d; k++) stage[m * d + k * m + r] = omega[r * d + k];
  return to_device(cb->e, b.om, stage.data(), stage.size());
}

// Step 2: b.xt <- the run's samples and b.vt <- the rows, projected by b.om
static int gmlvq_project_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const GmlvqBufs &b) {
  somhip_engine *e = cb->e;
  const unsigned ry = (unsigned)((b.d4m * 4 + 4 * GMLVQ_RT - 1) / (4 * GMLVQ_RT));
  CHK(LAUNCH_TIMED(e, KID_GMLVQ_PROJECT, (k_gmlvq_project<GLVQ_S, GMLVQ_RT>), dim3((unsigned)((n + WAVE - 1) / WAVE), ry), dim3(256), 0, b.om, cb->v.d, b.m,
      b.d4m, ds->d_rows, ds->n, first % ds->n, CbView{}, n, b.xt, nullptr, nullptr));
  return LAUNCH_TIMED(e, KID_GMLVQ_PROJECT, (k_gmlvq_project<GLVQ_S, GMLVQ_RT>), dim3((unsigned)cb->v.ngroups, ry), dim3(256), 0, b.om, cb->v.d, b.m, b.d4m,
                      nullptr, 0, 0, cb->v, cb->v.n, nullptr, b.vt, nullptr);
}
// Step 3: b.g.keys2 <- the two keys of every sample of the run: the class-wise scan's walk over the projected tiles, which
// packs nothing, under K9's id
static int gmlvq_search_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const GmlvqBufs &b) {
  HIPCHK(hipMemsetAsync(b.g.keys2, 0xFF, sizeof(uint64_t) * 2 * (size_t)n, cb->e->stream));
  return class_scan_walk(cb->e, b.pv, cb->d_labels, ds, first, n, /*projected*/ reinterpret_cast<const float4 *>(b.xt), /*sel*/ nullptr,
                         /*lam*/ nullptr, KID_GLVQ_SEARCH, b.g.keys2);
}
// Step 7: b.Gm from the terms, the winners and both projections
static int gmlvq_grad_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const GmlvqBufs &b) {
  somhip_engine *e = cb->e;
  const int64_t len = (int64_t)b.m * cb->v.d;
  LaunchTimer t(e, KID_GMLVQ_GRAD);
  const dim3 grid((unsigned)((cb->v.d + GMLVQ_THREADS - 1) / GMLVQ_THREADS), (unsigned)((b.m + GMLVQ_RT - 1) / GMLVQ_RT), (unsigned)b.nblocks);
  CHK(LAUNCH(e, (k_gmlvq_omega_grad<GMLVQ_RT, GMLVQ_AHEAD>), grid, dim3(GMLVQ_THREADS), 0, cb->v, b.pv, ds->d_rows, ds->n, first % ds->n, n, b.xt, b.g.win,
      b.g.xi, b.part));
  return LAUNCH(e, k_gmlvq_omega_reduce<GMLVQ_AHEAD>, dim3((unsigned)((len + GMLVQ_THREADS - 1) / GMLVQ_THREADS)), dim3(GMLVQ_THREADS), 0, b.part, b.nblocks,
                len, b.Gm);
}
// Step 6: the rows from b.g.S, b.g.hits and b.om
static int gmlvq_update_stage(somhip_codebook *cb, float alpha_t, int64_t n, const GmlvqBufs &b) {
  rows_written(cb);
  return LAUNCH_TIMED(cb->e, KID_GMLVQ_UPDATE, k_gmlvq_update<GMLVQ_THREADS>, dim3((unsigned)cb->v.n), dim3(GMLVQ_THREADS), 0, cb->v, b.g.S, b.g.hits, b.om,
                      b.omT, b.m, b.gbuf, b.P, (double)alpha_t / (double)n);
}
// Step 8 on the host, IEEE fp64: omega <- the step along -Gm, scaled to trace(Omega^T Omega) = 1; nothing where eps_t is 0
// or the step lands on the zero matrix
static void gmlvq_omega_step(float *omega, size_t len, const double *Gm, float eps_t, int64_t n) {
  if (!(eps_t > 0.0f)) return;
  const double e = (double)eps_t / (double)n;
  std::vector<double> O(len);
  double s = 0.0;
  for (size_t i = 0; i < len; i++) {
    const double step = e * Gm[i];
    const double v = (double)omega[i] - step;
    O[i] = v;
    const double vv = v * v;
    s += vv;
  }
  if (!(s > 0.0)) return;
  const double root = std::sqrt(s);
  for (size_t i = 0; i < len; i++) omega[i] = (float)(O[i] / root);
}

extern "C" int somhip_gmlvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_gmlvq_params *p, float *omega,
                                  double *cost_out, int64_t *correct_out) try {
  const char *who = "somhip_gmlvq_train";
  if (!p) return fail("%s: null parameters", who);
  if (!cb || !ds) return fail("%s: null handle", who);
  CHK(check_epochs(p->epochs, who));
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  CHK(check_alpha(p->alpha, who));
  CHK(glvq_check_beta(p->sigmoid_beta, who));
  CHK(grlvq_check_eps(p->eps, who));
  CHK(glvq_check(cb, ds, p->first, p->n, who));
  CHK(gmlvq_check_omega(omega, p->rank, cb->v.d, true, who));
  somhip_engine *e = cb->e;
  GmlvqBufs b;
  CHK(gmlvq_bind(cb, p->n, p->rank, &b));
  const size_t len = (size_t)p->rank * cb->v.d;
  std::vector<double> hc((size_t)(cost_out ? cb->v.n : 0)), Gm(len);
  std::vector<float> stage, om(omega, omega + len);
  for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
    const float alpha_t = linear_rate(p->alpha, p->epochs, t), eps_t = linear_rate(p->eps, p->epochs, t);
    CHK(gmlvq_put_omega(cb, om.data(), stage, b));
    CHK(gmlvq_project_stage(cb, ds, p->first, p->n, b));
    CHK(gmlvq_search_stage(cb, ds, p->first, p->n, b));
    CHK(glvq_terms_stage(cb, p->n, p->sigmoid_beta, b.g));
    CHK(glvq_sums_stage(cb, ds, p->first, p->n, b.g));
    if (eps_t > 0.0f) CHK(gmlvq_grad_stage(cb, ds, p->first, p->n, b));
    uint32_t correct = 0;
    if (cost_out) CHK(to_host(e, hc.data(), b.g.cost, hc.size()));
    if (correct_out) CHK(to_host(e, &correct, b.g.correct, 1));
    if (eps_t > 0.0f) CHK(to_host(e, Gm.data(), b.Gm, len));
    CHK(gmlvq_update_stage(cb, alpha_t, p->n, b));                      // (with the omega the epoch started from, on the device)
    HIPCHK(hipStreamSynchronize(e->stream));                            // (the copies have landed; `stage` may be rewritten)
    if (cost_out) cost_out[t - p->start_epoch] = cost_figure(hc, (double)p->n);
    if (correct_out) correct_out[t - p->start_epoch] = (int64_t)correct;
    gmlvq_omega_step(om.data(), len, Gm.data(), eps_t, p->n);
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  std::copy(om.begin(), om.end(), omega);
  return 0;
} ABI_CATCH(somhip_gmlvq_train)

extern "C" int somhip_gmlvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *omega, int32_t rank,
                                   float *dplus, int32_t *iplus, float *dminus, int32_t *iminus) try {
  const char *who = "somhip_gmlvq_search";
  if (!dplus || !iplus || !dminus || !iminus) return fail("%s: null output", who);
  CHK(glvq_check(cb, ds, first, n, who));
  CHK(gmlvq_check_omega(omega, rank, cb->v.d, false, who));
  somhip_engine *e = cb->e;
  GmlvqBufs b;
  CHK(gmlvq_bind(cb, n, rank, &b));
  std::vector<float> stage;
  CHK(gmlvq_put_omega(cb, omega, stage, b));
  CHK(gmlvq_project_stage(cb, ds, first, n, b));
  CHK(gmlvq_search_stage(cb, ds, first, n, b));
  return glvq_keys_to_host(e, b.g, n, dplus, iplus, dminus, iminus);
} ABI_CATCH(somhip_gmlvq_search)

extern "C" int somhip_gmlvq_project(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *omega, int32_t rank,
                                    float *out) try {
  const char *who = "somhip_gmlvq_project";
  if (!out) return fail("%s: null output", who);
  if (ds) {
    CHK(check_pair(cb, ds, who));
    if (ds->d_mask) return fail("%s: data with masked components (x) is not supported", who);
    if (first < 0) return fail("%s: first row %lld < 0", who, (long long)first);
    if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  } else {
    CHK(check_codebook(cb, true, who));
    if (is_shard(cb)) return fail("%s: sharded codebook not supported (a shard does not hold the other shards' rows)", who);
    n = cb->v.n;
  }
  CHK(gmlvq_check_omega(omega, rank, cb->v.d, false, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const size_t len = (size_t)rank * cb->v.d;
  float *om, *flat;
  CHK(scratch(e, SLOT_GMLVQ, len, &om));
  CHK(scratch(e, SLOT_GMLVQ_PART, (size_t)n * rank, &flat));
  CHK(to_device(e, om, omega, len));
  const int d4m = (rank + 3) / 4;
  const unsigned ry = (unsigned)((d4m * 4 + 4 * GMLVQ_RT - 1) / (4 * GMLVQ_RT));
  if (ds)
    CHK(LAUNCH_TIMED(e, KID_GMLVQ_PROJECT, (k_gmlvq_project<GLVQ_S, GMLVQ_RT>), dim3((unsigned)((n + WAVE - 1) / WAVE), ry), dim3(256), 0, om, cb->v.d, rank,
        d4m, ds->d_rows, ds->n, first % ds->n, CbView{}, n, nullptr, nullptr, flat));
  else
    CHK(LAUNCH_TIMED(e, KID_GMLVQ_PROJECT, (k_gmlvq_project<GLVQ_S, GMLVQ_RT>), dim3((unsigned)cb->v.ngroups, ry), dim3(256), 0, om, cb->v.d, rank, d4m,
        nullptr, 0, 0, cb->v, n, nullptr, nullptr, flat));
  return to_host_sync(e, out, flat, (size_t)n * rank);
} ABI_CATCH(somhip_gmlvq_project)

extern "C" int somhip_debug_gmlvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta,
                                       const float *omega, int32_t rank, double *xi_plus, double *xi_minus, double *f,
                                       double *sums_plus, uint32_t *n_plus, double *sums_minus, uint32_t *n_minus, double *cost,
                                       int64_t *correct, double *grad) try {
  const char *who = "somhip_debug_gmlvq_sums";
  if (!xi_plus || !xi_minus || !f || !sums_plus || !n_plus || !sums_minus || !n_minus || !cost || !correct || !grad) return fail("%s: null output", who);
  CHK(glvq_check_beta(sigmoid_beta, who));
  CHK(glvq_check(cb, ds, first, n, who));
  CHK(gmlvq_check_omega(omega, rank, cb->v.d, false, who));
  somhip_engine *e = cb->e;
  GmlvqBufs b;
  CHK(gmlvq_bind(cb, n, rank, &b));
  std::vector<float> stage;
  CHK(gmlvq_put_omega(cb, omega, stage, b));
  CHK(gmlvq_project_stage(cb, ds, first, n, b));
  CHK(gmlvq_search_stage(cb, ds, first, n, b));
  CHK(glvq_terms_stage(cb, n, sigmoid_beta, b.g));
  CHK(glvq_sums_stage(cb, ds, first, n, b.g));
  CHK(gmlvq_grad_stage(cb, ds, first, n, b));
  uint32_t hcorrect = 0;
  CHK(glvq_sums_to_host(cb, b.g, n, xi_plus, xi_minus, f, sums_plus, n_plus, sums_minus, n_minus, cost));
  CHK(to_host(e, grad, b.Gm, (size_t)rank * cb->v.d));
  CHK(to_host_sync(e, &hcorrect, b.g.correct, 1));
  *correct = (int64_t)hcorrect;
  return 0;
} ABI_CATCH(somhip_debug_gmlvq_sums)

extern "C" int somhip_debug_gmlvq_update(somhip_codebook *cb, float alpha_t, float eps_t, int64_t n, float *omega, int32_t rank,
                                         const double *sums_plus, const uint32_t *n_plus, const double *sums_minus,
                                         const uint32_t *n_minus, const double *grad) try {
  const char *who = "somhip_debug_gmlvq_update";
  CHK(check_codebook(cb, sums_plus && n_plus && sums_minus && n_minus && grad, who));
  CHK(glvq_check_codebook(cb, who));
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  CHK(grlvq_check_eps(eps_t, who));
  CHK(gmlvq_check_omega(omega, rank, cb->v.d, false, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  GmlvqBufs b;
  CHK(gmlvq_bind(cb, 0, rank, &b));
  std::vector<float> stage;
  CHK(gmlvq_put_omega(cb, omega, stage, b));
  CHK(glvq_sums_to_device(cb, b.g, sums_plus, n_plus, sums_minus, n_minus));
  CHK(gmlvq_update_stage(cb, alpha_t, n, b));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (the host arrays are read until the copies have run)
  gmlvq_omega_step(omega, (size_t)rank * cb->v.d, grad, eps_t, n);
  return 0;
} ABI_CATCH(somhip_debug_gmlvq_update)

// HIP-event totals of the stages since somhip_timing_reset, while somhip_timing_enable is on: [0] the projections, [1] the
// class-wise scan, [2] terms and grouping, [3] sums (these three K9's stages under K9's ids), [4] the gradient of Omega with
// its reduction, [5] update
extern "C" int somhip_gmlvq_timing(somhip_engine *e, int64_t launches[6], double total_ms[6]) try {
  const int kid[6] = {KID_GMLVQ_PROJECT, KID_GLVQ_SEARCH, KID_GLVQ_TERMS, KID_GLVQ_SUMS, KID_GMLVQ_GRAD, KID_GMLVQ_UPDATE};
  return stage_timing(e, "somhip_gmlvq_timing", kid, 6, launches, total_ms);
} ABI_CATCH(somhip_gmlvq_timing)
