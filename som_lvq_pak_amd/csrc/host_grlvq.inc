// host_grlvq.inc -- K11, batch GRLVQ: K9's epoch under the relevance-weighted metric -- the weighted class-wise search, K9's
// terms and grouping (unchanged), the sums with the relevance chain, the ordered reduction of the relevance gradient over
// the rows, the weighted update, and the relevance step on the host; the stages on their own for the tests
// (included by somhip.hip behind host_glvq.inc: one translation unit; K9's checks, binding, terms stage by name, and the
// trainers' shared pieces of host_proto.inc: the class-wise scan's walk with the relevance tile, the family's copies)

// The device arrays of a GRLVQ call beside K9's (GlvqBufs: SLOT_GLVQ, SLOT_GLVQ_LIST).  SLOT_GRLVQ: [lam: d4 float4, the
// padding zero][R: 2 x rows x dim doubles][G: dim doubles].  R is what makes the feature large: 16 bytes per row and
// component (100 000 x 1024: 1.6 GB).
struct GrlvqBufs {
  GlvqBufs g;
  double *R = nullptr, *G = nullptr;
  float4 *lam = nullptr;
};
static int grlvq_bind(somhip_codebook *cb, int64_t n, GrlvqBufs *b) {
  CHK(glvq_bind(cb, n, &b->g));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  void *p;
  CHK(engine_scratch(cb->e, SLOT_GRLVQ, sizeof(double) * (2 * units * d + d) + sizeof(float4) * (size_t)cb->v.d4, &p));
  b->lam = (float4 *)p;                                   // (first: 16-byte aligned)
  b->R = reinterpret_cast<double *>(b->lam + cb->v.d4);
  b->G = b->R + 2 * units * d;
  return 0;
}

// what every entry point asks of a relevance vector before anything is launched
static int grlvq_check_lambda(const float *lambda, int d, bool nonzero, const char *who) {
  if (!lambda) return fail("%s: null lambda", who);
  double s = 0.0;
  for (int k = 0; k < d; k++) {
    if (!(lambda[k] >= 0.0f) || std::isinf(lambda[k]))
      return fail("%s: lambda[%d] = %g is negative or not a finite number", who, k, (double)lambda[k]);
    s += (double)lambda[k];
  }
  if (nonzero && !(s > 0.0)) return fail("%s: lambda sums to zero (every distance would be 0)", who);
  return 0;
}
static int grlvq_check_eps(float eps, const char *who) {
  return eps >= 0.0f ? 0 : fail("%s: eps %g is negative or not a number", who, (double)eps);
}

// lambda -> b.lam through `tile` (d4 * 4 floats the caller keeps until the stream has been waited for)
static int grlvq_put_lambda(somhip_codebook *cb, const float *lambda, std::vector<float> &tile, const GrlvqBufs &b) {
  tile.assign((size_t)cb->v.d4 * 4, 0.0f);
  std::copy(lambda, lambda + cb->v.d, tile.begin());
  return to_device(cb->e, reinterpret_cast<float *>(b.lam), tile.data(), tile.size());
}

// Step 2: b.g.keys2 <- the two keys of every sample of the run under b.lam: the class-wise scan's walk, weighted
static int grlvq_search_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const GrlvqBufs &b) {
  HIPCHK(hipMemsetAsync(b.g.keys2, 0xFF, sizeof(uint64_t) * 2 * (size_t)n, cb->e->stream));
  return class_scan_walk(cb->e, cb->v, cb->d_labels, ds, first, n, /*projected*/ nullptr, /*sel*/ nullptr, /*lam*/ b.lam, KID_GRLVQ_SEARCH, b.g.keys2);
}
// Step 4: b.g.S, b.g.cost and b.R from the lists; step 5: b.G from b.R
static int grlvq_sums_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const GrlvqBufs &b) {
  const dim3 grid((unsigned)cb->v.n, (unsigned)((cb->v.d + 2 + BM_SUM_DIMS - 1) / BM_SUM_DIMS), 2);
  CHK(LAUNCH_TIMED(cb->e, KID_GRLVQ_SUMS, k_grlvq_sums<GLVQ_SUM_AHEAD>, grid, dim3(BM_SUM_DIMS), 0, cb->v, ds->d_rows, ds->n, first % ds->n, n, b.g.list,
      b.g.starts, b.g.xi, b.g.f, b.g.S, b.R, b.g.cost));
  return LAUNCH_TIMED(cb->e, KID_GRLVQ_RELEVANCE, k_grlvq_relevance<GRLVQ_RED_AHEAD>, dim3((unsigned)((cb->v.d + WAVE - 1) / WAVE)), dim3(WAVE), 0, b.R,
                      (uint32_t)cb->v.n, cb->v.d, b.G);
}
// Step 6: the rows from b.g.S, b.g.hits and b.lam
static int grlvq_update_stage(somhip_codebook *cb, float alpha_t, int64_t n, const GrlvqBufs &b) {
  const int64_t threads = cb->v.ngroups * cb->v.d4 * WAVE;
  rows_written(cb);
  return LAUNCH_TIMED(cb->e, KID_GRLVQ_UPDATE, k_grlvq_update<GLVQ_THREADS>, dim3((unsigned)((threads + GLVQ_THREADS - 1) / GLVQ_THREADS)), dim3(GLVQ_THREADS), 0,
                      cb->v, b.g.S, b.g.hits, reinterpret_cast<const float *>(b.lam), (double)alpha_t / (double)n);
}
// Step 7 on the host, IEEE fp64: lambda <- the clamped, normalised step along -G; nothing where eps_t is 0 or every
// component is clamped
static void grlvq_relevance_step(float *lambda, int d, const double *G, float eps_t, int64_t n) {
  if (!(eps_t > 0.0f)) return;
  const double e = (double)eps_t / (2.0 * (double)n);
  std::vector<double> l((size_t)d);
  double s = 0.0;
  for (int k = 0; k < d; k++) {
    const double step = e * G[k];
    double v = (double)lambda[k] - step;
    if (v < 0.0) v = 0.0;
    l[(size_t)k] = v;
    s += v;
  }
  if (!(s > 0.0)) return;
  for (int k = 0; k < d; k++) lambda[k] = (float)(l[(size_t)k] / s);
}

extern "C" int somhip_grlvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_grlvq_params *p, float *lambda,
                                  double *cost_out, int64_t *correct_out) try {
  const char *who = "somhip_grlvq_train";
  if (!p) return fail("%s: null parameters", who);
  if (!cb || !ds) return fail("%s: null handle", who);
  CHK(check_epochs(p->epochs, who));
  CHK(check_epoch_window(p->start_epoch, p->count, p->epochs, who));
  CHK(check_alpha(p->alpha, who));
  CHK(glvq_check_beta(p->sigmoid_beta, who));
  CHK(grlvq_check_eps(p->eps, who));
  CHK(glvq_check(cb, ds, p->first, p->n, who));
  CHK(grlvq_check_lambda(lambda, cb->v.d, true, who));
  somhip_engine *e = cb->e;
  GrlvqBufs b;
  CHK(grlvq_bind(cb, p->n, &b));
  const int d = cb->v.d;
  std::vector<double> hc((size_t)(cost_out ? cb->v.n : 0)), G((size_t)d);
  std::vector<float> tile, lam(lambda, lambda + d);
  for (int64_t t = p->start_epoch; t < p->start_epoch + p->count; t++) {
    const float alpha_t = linear_rate(p->alpha, p->epochs, t), eps_t = linear_rate(p->eps, p->epochs, t);
    CHK(grlvq_put_lambda(cb, lam.data(), tile, b));
    CHK(grlvq_search_stage(cb, ds, p->first, p->n, b));
    CHK(glvq_terms_stage(cb, p->n, p->sigmoid_beta, b.g));
    CHK(grlvq_sums_stage(cb, ds, p->first, p->n, b));
    uint32_t correct = 0;
    if (cost_out) CHK(to_host(e, hc.data(), b.g.cost, hc.size()));
    if (correct_out) CHK(to_host(e, &correct, b.g.correct, 1));
    CHK(to_host_sync(e, G.data(), b.G, G.size()));
    if (cost_out) cost_out[t - p->start_epoch] = cost_figure(hc, (double)p->n);
    if (correct_out) correct_out[t - p->start_epoch] = (int64_t)correct;
    CHK(grlvq_update_stage(cb, alpha_t, p->n, b));                      // (with the lambda the epoch started from, on the device)
    grlvq_relevance_step(lam.data(), d, G.data(), eps_t, p->n);
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  std::copy(lam.begin(), lam.end(), lambda);
  return 0;
} ABI_CATCH(somhip_grlvq_train)

extern "C" int somhip_grlvq_search(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, const float *lambda,
                                   float *dplus, int32_t *iplus, float *dminus, int32_t *iminus) try {
  const char *who = "somhip_grlvq_search";
  if (!dplus || !iplus || !dminus || !iminus) return fail("%s: null output", who);
  CHK(glvq_check(cb, ds, first, n, who));
  CHK(grlvq_check_lambda(lambda, cb->v.d, false, who));
  somhip_engine *e = cb->e;
  GrlvqBufs b;
  CHK(grlvq_bind(cb, n, &b));
  std::vector<float> tile;
  CHK(grlvq_put_lambda(cb, lambda, tile, b));
  CHK(grlvq_search_stage(cb, ds, first, n, b));
  return glvq_keys_to_host(e, b.g, n, dplus, iplus, dminus, iminus);
} ABI_CATCH(somhip_grlvq_search)

extern "C" int somhip_debug_grlvq_sums(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta,
                                       const float *lambda, double *xi_plus, double *xi_minus, double *f, double *sums_plus,
                                       uint32_t *n_plus, double *sums_minus, uint32_t *n_minus, double *cost, int64_t *correct,
                                       double *rel_plus, double *rel_minus, double *grad) try {
  const char *who = "somhip_debug_grlvq_sums";
  if (!xi_plus || !xi_minus || !f || !sums_plus || !n_plus || !sums_minus || !n_minus || !cost || !correct || !rel_plus || !rel_minus || !grad)
    return fail("%s: null output", who);
  CHK(glvq_check_beta(sigmoid_beta, who));
  CHK(glvq_check(cb, ds, first, n, who));
  CHK(grlvq_check_lambda(lambda, cb->v.d, false, who));
  somhip_engine *e = cb->e;
  GrlvqBufs b;
  CHK(grlvq_bind(cb, n, &b));
  std::vector<float> tile;
  CHK(grlvq_put_lambda(cb, lambda, tile, b));
  CHK(grlvq_search_stage(cb, ds, first, n, b));
  CHK(glvq_terms_stage(cb, n, sigmoid_beta, b.g));
  CHK(grlvq_sums_stage(cb, ds, first, n, b));
  const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
  uint32_t hcorrect = 0;
  CHK(glvq_sums_to_host(cb, b.g, n, xi_plus, xi_minus, f, sums_plus, n_plus, sums_minus, n_minus, cost));
  CHK(to_host(e, rel_plus, b.R, units * d));
  CHK(to_host(e, rel_minus, b.R + units * d, units * d));
  CHK(to_host(e, grad, b.G, d));
  CHK(to_host_sync(e, &hcorrect, b.g.correct, 1));
  *correct = (int64_t)hcorrect;
  return 0;
} ABI_CATCH(somhip_debug_grlvq_sums)

extern "C" int somhip_debug_grlvq_update(somhip_codebook *cb, float alpha_t, float eps_t, int64_t n, float *lambda,
                                         const double *sums_plus, const uint32_t *n_plus, const double *sums_minus,
                                         const uint32_t *n_minus, const double *grad) try {
  const char *who = "somhip_debug_grlvq_update";
  CHK(check_codebook(cb, sums_plus && n_plus && sums_minus && n_minus && grad, who));
  CHK(glvq_check_codebook(cb, who));
  if (n <= 0) return fail("%s: n %lld <= 0", who, (long long)n);
  CHK(grlvq_check_eps(eps_t, who));
  CHK(grlvq_check_lambda(lambda, cb->v.d, false, who));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  GrlvqBufs b;
  CHK(grlvq_bind(cb, 0, &b));
  std::vector<float> tile;
  CHK(grlvq_put_lambda(cb, lambda, tile, b));
  CHK(glvq_sums_to_device(cb, b.g, sums_plus, n_plus, sums_minus, n_minus));
  CHK(grlvq_update_stage(cb, alpha_t, n, b));
  HIPCHK(hipStreamSynchronize(e->stream));                              // (the host arrays are read until the copies have run)
  grlvq_relevance_step(lambda, cb->v.d, grad, eps_t, n);
  return 0;
} ABI_CATCH(somhip_debug_grlvq_update)

// HIP-event totals of the stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own behind the
// published table, but for the terms, which are K9's stage under K9's id): [0] search, [1] terms and grouping, [2] sums,
// [3] the relevance reduction, [4] update
extern "C" int somhip_grlvq_timing(somhip_engine *e, int64_t launches[5], double total_ms[5]) try {
  const int kid[5] = {KID_GRLVQ_SEARCH, KID_GLVQ_TERMS, KID_GRLVQ_SUMS, KID_GRLVQ_RELEVANCE, KID_GRLVQ_UPDATE};
  return stage_timing(e, "somhip_grlvq_timing", kid, 5, launches, total_ms);
} ABI_CATCH(somhip_grlvq_timing)
