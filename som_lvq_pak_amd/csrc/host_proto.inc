// host_proto.inc -- what the batch prototype trainers share on the host (K8 the batch map, K9 GLVQ, K10 / K10d neural gas,
// K11 GRLVQ, K12 GMLVQ, K13 RSLVQ): the refusals of an epoch window and the linear rate, the class-wise scan's walk over
// its chunks, the copies of the GLVQ family's debug entry points, the cost figure, the trailing column of a [rows][d + 1]
// matrix, and the distance and sums stages of a chunk that RSLVQ and the dense neural gas both run
// (included by somhip.hip ahead of host_batchmap.inc: one translation unit; rows_written and stage_timing, which the SOM
// and LVQ drivers use as well, are in somhip.hip)

// ---------------------------------------------------------------------------------
// epochs [start, start + count) of `epochs`, and the rate of epoch t: each check on its own, so that an entry point keeps
// the order of its refusals
// ---------------------------------------------------------------------------------
static int check_epochs(int64_t epochs, const char *who) {
  return epochs >= 1 ? 0 : fail("%s: epochs %lld < 1", who, (long long)epochs);
}
static int check_epoch_window(int64_t start, int64_t count, int64_t epochs, const char *who) {
  if (start < 0 || count < 0 || start + count > epochs)
    return fail("%s: epochs [%lld, %lld) outside [0, %lld)", who, (long long)start, (long long)(start + count), (long long)epochs);
  return 0;
}
static int check_alpha(float alpha, const char *who) {
  return alpha >= 0.0f ? 0 : fail("%s: alpha %g is negative or not a number", who, (double)alpha);
}
// LVQ_PAK's linear rate over epochs (som_rout.c:615 for a radius above 1): float throughout, in this order
static float linear_rate(float alpha, int64_t epochs, int64_t t) { return alpha * (float)(epochs - t) / (float)epochs; }

// ---------------------------------------------------------------------------------
// the class-wise scan (kernels/glvq.hpp): K9's search, K11's under a relevance vector, K12's over projected tiles
// ---------------------------------------------------------------------------------
constexpr int64_t GLVQ_CHUNK = 16384;           // samples of a class-wise scan launch: whole tiles (dim 1024: 64 MiB of sample tiles)

// keys2 (which holds KEY_NONE for them) <- the two keys of `count` samples of the run that starts at data row `first`
// against the rows of v, in chunks of whole sample tiles; the sample labels are on the device.  The samples are the run's
// own 0 .. count - 1, or the listed ones sel[0 .. count).  Their tiles: `projected` (the whole run's, v.d4 wide, made by the
// caller), else packed chunk by chunk into SLOT_SAMPLES -- the run's by k_pack_samples under its own id, the listed ones
// by k_glvq_pack_listed untimed.  lam (or null): the relevance tile, which selects the weighted kernel (it takes no list).
// kid: the id the scan's launches count under, -1 for none (K9's list route times one span around everything instead).
static int class_scan_walk(somhip_engine *e, const CbView &v, const int32_t *row_labels, somhip_dataset *ds, int64_t first, int64_t count,
                           const float4 *projected, const uint32_t *sel, const float4 *lam, int kid, uint64_t *keys2) {
  const int64_t f0 = first % ds->n;
  const bool wide = v.ngroups >= 4 * GLVQ_R;
  const dim3 block(256);
  for (int64_t off = 0; off < count; off += GLVQ_CHUNK) {
    const int64_t c = std::min(GLVQ_CHUNK, count - off), nsb = (c + GLVQ_S - 1) / GLVQ_S;
    const float4 *xt = projected ? projected + (off / GLVQ_S) * v.d4 * GLVQ_S : nullptr;
    if (!xt) {
      float4 *packed;
      CHK(scratch(e, SLOT_SAMPLES, (size_t)nsb * v.d4 * GLVQ_S, &packed));
      if (sel)
        CHK(LAUNCH(e, k_glvq_pack_listed<GLVQ_S>, dim3((unsigned)nsb), block, 0, ds->d_rows, ds->n, ds->d, v.d4, f0, sel + off, c, packed));
      else
        CHK(LAUNCH_TIMED(e, KID_PACK_SAMPLES, k_pack_samples<GLVQ_S>, dim3((unsigned)nsb), block, 0, ds->d_rows, ds->n, ds->d, v.d4,
            (f0 + off) % ds->n, c, packed));
      xt = packed;
    }
    const dim3 grid((unsigned)nsb, (unsigned)((v.ngroups + (wide ? 4 * GLVQ_R : 4) - 1) / (wide ? 4 * GLVQ_R : 4)));
    const uint32_t *sl = sel ? sel + off : nullptr;
    if (lam && wide)
      CHK(LAUNCH_TIMED(e, kid, (k_scan_class_weighted<GLVQ_S, GLVQ_R>), grid, block, 0, v, xt, lam, c, row_labels, ds->d_labels, ds->n, f0, off, keys2));
    else if (lam)
      CHK(LAUNCH_TIMED(e, kid, (k_scan_class_weighted<GLVQ_S, 1>), grid, block, 0, v, xt, lam, c, row_labels, ds->d_labels, ds->n, f0, off, keys2));
    else if (wide)
      CHK(LAUNCH_TIMED(e, kid, (k_scan_class<GLVQ_S, GLVQ_R>), grid, block, 0, v, xt, c, row_labels, ds->d_labels, ds->n, f0, off, sl, keys2));
    else
      CHK(LAUNCH_TIMED(e, kid, (k_scan_class<GLVQ_S, 1>), grid, block, 0, v, xt, c, row_labels, ds->d_labels, ds->n, f0, off, sl, keys2));
  }
  e->samples_searched += (uint64_t)count;
  return 0;
}

// ---------------------------------------------------------------------------------
// the GLVQ family's arrays (K9, K11 and K12 bind them with glvq_bind, host_glvq.inc) and their copies
// ---------------------------------------------------------------------------------
// The device arrays of a GLVQ call.  SLOT_GLVQ, per row: [S: 2 x rows x (dim + 1) doubles][cost][hits: 2 x rows]
// [starts: 2 x (rows + 1)][correct, the remainder's length].  SLOT_GLVQ_LIST, per sample: [keys2][xi: 2 x n][f][win: 2 x n]
// [idx][the sorted winners][list: 2 x n][the remainder][the sort's own room].  Role + comes first in every pair.
struct GlvqBufs {
  double *S = nullptr, *cost = nullptr, *xi = nullptr, *f = nullptr;
  uint64_t *keys2 = nullptr;
  uint32_t *hits = nullptr, *starts = nullptr, *correct = nullptr, *rem_count = nullptr;
  uint32_t *win = nullptr, *idx = nullptr, *win_sorted = nullptr, *list = nullptr, *rem = nullptr;
  void *sort_tmp = nullptr;
  size_t sort_bytes = 0;
  unsigned sort_bits = 0;
};

// what a search entry point returns: b.keys2 of n samples as (dplus, iplus, dminus, iminus), waited for
static int glvq_keys_to_host(somhip_engine *e, const GlvqBufs &b, int64_t n, float *dplus, int32_t *iplus, float *dminus, int32_t *iminus) {
  std::vector<uint64_t> hk(2 * (size_t)n);
  CHK(to_host_sync(e, hk.data(), b.keys2, hk.size()));
  for (int64_t s = 0; s < n; s++) {
    decode_key(hk[2 * (size_t)s], false, iplus + s, dplus + s);
    decode_key(hk[2 * (size_t)s + 1], false, iminus + s, dminus + s);
  }
  return 0;
}
// what a *_debug_*_sums entry point returns of K9's terms and sums, but for b.correct: queued, not waited for -- the
// caller queues its own arrays behind these, then the word of b.correct with the one wait (to_host_sync)
static int glvq_sums_to_host(somhip_codebook *cb, const GlvqBufs &b, int64_t n, double *xi_plus, double *xi_minus, double *f, double *sums_plus,
                             uint32_t *n_plus, double *sums_minus, uint32_t *n_minus, double *cost) {
  somhip_engine *e = cb->e;
  const size_t units = (size_t)cb->v.n, ld = (size_t)cb->v.d + 1, ns = (size_t)n;
  CHK(to_host(e, xi_plus, b.xi, ns));
  CHK(to_host(e, xi_minus, b.xi + ns, ns));
  CHK(to_host(e, f, b.f, ns));
  CHK(to_host(e, sums_plus, b.S, units * ld));
  CHK(to_host(e, sums_minus, b.S + units * ld, units * ld));
  CHK(to_host(e, n_plus, b.hits, units));
  CHK(to_host(e, n_minus, b.hits + units, units));
  return to_host(e, cost, b.cost, units);
}
// what a *_debug_*_update entry point takes: the sums and counts of both roles into b.S and b.hits, queued (the host
// arrays are read until the stream has been waited for)
static int glvq_sums_to_device(somhip_codebook *cb, const GlvqBufs &b, const double *sums_plus, const uint32_t *n_plus, const double *sums_minus,
                               const uint32_t *n_minus) {
  somhip_engine *e = cb->e;
  const size_t units = (size_t)cb->v.n, ld = (size_t)cb->v.d + 1;
  CHK(to_device(e, b.S, sums_plus, units * ld));
  CHK(to_device(e, b.S + units * ld, sums_minus, units * ld));
  CHK(to_device(e, b.hits, n_plus, units));
  return to_device(e, b.hits + units, n_minus, units);
}
// The cost figure of an epoch from the terms a driver has copied to the host (K9: per row; K13: per sample) and waited
// for: the fp64 chain in array order / samples.  Queueing the copy stays with the driver, beside its other copies.
static double cost_figure(const std::vector<double> &terms, double samples) {
  double chain = 0.0;
  for (double c : terms) chain += c;
  return chain / samples;
}

// ---------------------------------------------------------------------------------
// [rows][d + 1] doubles on the device side of a debug entry point <-> the matrix [rows][d] and the trailing column
// (or null: not wanted) on its caller's
// ---------------------------------------------------------------------------------
static void split_trailing(const double *packed, size_t rows, size_t d, double *matrix, double *column) {
  for (size_t r = 0; r < rows; r++) {
    memcpy(matrix + r * d, packed + r * (d + 1), sizeof(double) * d);
    if (column) column[r] = packed[r * (d + 1) + d];
  }
}
static void join_trailing(double *packed, size_t rows, size_t d, const double *matrix, const double *column) {
  for (size_t r = 0; r < rows; r++) {
    memcpy(packed + r * (d + 1), matrix + r * d, sizeof(double) * d);
    packed[r * (d + 1) + d] = column[r];
  }
}

// ---------------------------------------------------------------------------------
// a chunk of c samples of the run from `off` on, for K13 and K10d: every exact distance, and Q^T x [X | 1] on the fp64 MFMA
// ---------------------------------------------------------------------------------
// dist [c][ld] <- the distances to every row (k_pack_samples, K1w's k_knn_dist, unchanged), both under kid
static int dist_chunk_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t off, int64_t c, int kid, int64_t ld, float *dist) {
  somhip_engine *e = cb->e;
  const int64_t nsb = (c + SCAN_S - 1) / SCAN_S;
  float4 *xt;
  CHK(scratch(e, SLOT_SAMPLES, (size_t)nsb * cb->v.d4 * SCAN_S, &xt));
  LaunchTimer t(e, kid);
  CHK(LAUNCH(e, k_pack_samples<SCAN_S>, dim3((unsigned)nsb), dim3(256), 0, ds->d_rows, ds->n, ds->d, cb->v.d4, (first % ds->n + off) % ds->n, c, xt));
  CHK(LAUNCH(e, k_knn_dist<SCAN_S>, dim3((unsigned)nsb, (unsigned)((cb->v.ngroups + 3) / 4)), dim3(256), 0, cb->v, xt, c, ld, dist));
  e->samples_searched += (uint64_t)c;
  return 0;
}
// acc [rows][dim + 1] <- the chains of Q [c][ld] over the chunk's rows, from +0.0 for the run's first chunk and from acc
// behind it (K13's k_rslvq_sums, called by both)
static int sums_chunk_stage(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t off, int64_t c, int kid, const double *Q, int64_t ld,
                            double *acc) {
  const dim3 grid((unsigned)cb->v.ngroups, (unsigned)((cb->v.d + RS_COLS - 1) / RS_COLS));
  const int64_t f = (first % ds->n + off) % ds->n;
  if (off > 0) return LAUNCH_TIMED(cb->e, kid, k_rslvq_sums<true>, grid, dim3(256), 0, Q, ld, c, ds->d_rows, ds->n, ds->d, f, cb->v.n, acc);
  return LAUNCH_TIMED(cb->e, kid, k_rslvq_sums<false>, grid, dim3(256), 0, Q, ld, c, ds->d_rows, ds->n, ds->d, f, cb->v.n, acc);
}
