// host_distortion.inc -- K1d, map distortion: the state (somhip_distortion: [S | hits], Q and the samples taken), the
// accumulation of a piece of data into it -- the batch map's group and continued sums stages on the state's S, then the two
// Q passes -- and the evaluation at a radius against the codebook's current rows
// (included by somhip.hip behind host_batchmap.inc: one translation unit, shared static helpers)

// The state, the caller's: device memory of one engine for one shape.  S is what somhip_batchmap_accumulate keeps in a
// codebook's own state, [S | hits] as units x (dim + 1) doubles; Q[units] beside it.  Behind them the room of an
// evaluation: the partials per (unit, column block), {D, A}, e_j and scale_j per unit, the two totals.
struct somhip_distortion {
  somhip_engine *e = nullptr;
  int64_t units = 0;
  int d = 0, nblk = 0;              // nblk: column blocks of the evaluate kernel
  uint64_t samples = 0;
  double *S = nullptr, *Q = nullptr;
  double *pe = nullptr, *pm = nullptr, *da = nullptr, *unit_e = nullptr, *unit_s = nullptr, *totals = nullptr;
  double *qs = nullptr;             // [qs_cap] |x_s|^2 of a piece's samples, kept between calls
  size_t qs_cap = 0;
};

static void distortion_release(somhip_distortion *st) {
  void *p[] = {st->S, st->Q, st->pe, st->pm, st->da, st->unit_e, st->unit_s, st->totals, st->qs};
  for (void *q : p) if (q) (void)hipFree(q);
  st->S = st->Q = st->pe = st->pm = st->da = st->unit_e = st->unit_s = st->totals = st->qs = nullptr;
  st->qs_cap = 0;
  st->samples = 0;
  st->e = nullptr;
}
static int check_distortion(const somhip_distortion *st, bool args, const char *who) {
  if (!st || !args) return fail("%s: null argument", who);
  if (!st->e) return fail("%s: the engine of this distortion state was destroyed", who);
  return 0;
}
// what the entry points on a state and a codebook refuse before anything is launched
static int distortion_check_codebook(const somhip_distortion *st, const somhip_codebook *cb, const char *who) {
  if (!cb) return fail("%s: null argument", who);
  if (!cb->e) return fail("%s: the engine of this codebook was destroyed", who);
  if (st && st->e != cb->e) return fail("%s: state and codebook belong to different engines", who);
  CHK(batchmap_check_codebook(cb, who));
  if (st && (st->units != cb->v.n || st->d != cb->v.d))
    return fail("%s: the state is of a %lld x %d codebook, this one is %lld x %d", who, (long long)st->units, st->d, (long long)cb->v.n, cb->v.d);
  return 0;
}
static int distortion_zero(somhip_distortion *st) {
  somhip_engine *e = st->e;
  HIPCHK(hipMemsetAsync(st->S, 0, sizeof(double) * (size_t)st->units * (size_t)(st->d + 1), e->stream));
  HIPCHK(hipMemsetAsync(st->Q, 0, sizeof(double) * (size_t)st->units, e->stream));
  st->samples = 0;
  return 0;
}
static int distortion_new(somhip_codebook *cb, somhip_distortion **out) {
  somhip_engine *e = cb->e;
  somhip_distortion *st = new somhip_distortion();
  st->e = e;
  st->units = cb->v.n;
  st->d = cb->v.d;
  st->nblk = (cb->v.d + BM_COLS - 1) / BM_COLS;
  e->distortions.push_back(st);
  auto fill = [&]() -> int {
    const size_t units = (size_t)st->units, nb = (size_t)st->nblk;
    HIPCHK(hipMalloc((void **)&st->S, sizeof(double) * units * (size_t)(st->d + 1)));
    HIPCHK(hipMalloc((void **)&st->Q, sizeof(double) * units));
    HIPCHK(hipMalloc((void **)&st->pe, sizeof(double) * units * nb));
    HIPCHK(hipMalloc((void **)&st->pm, sizeof(double) * units * nb));
    HIPCHK(hipMalloc((void **)&st->da, sizeof(double) * units * 2));
    HIPCHK(hipMalloc((void **)&st->unit_e, sizeof(double) * units));
    HIPCHK(hipMalloc((void **)&st->unit_s, sizeof(double) * units));
    HIPCHK(hipMalloc((void **)&st->totals, sizeof(double) * 2));
    CHK(distortion_zero(st));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
  };
  if (int rc = fill()) { somhip_distortion_destroy(st); return rc; }
  *out = st;
  return 0;
}

extern "C" int somhip_distortion_create(somhip_codebook *cb, somhip_distortion **out) try {
  CHK(check_codebook(cb, out, "somhip_distortion_create"));
  CHK(distortion_check_codebook(nullptr, cb, "somhip_distortion_create"));
  HIPCHK(hipSetDevice(cb->e->device));
  return distortion_new(cb, out);
} ABI_CATCH(somhip_distortion_create)
extern "C" void somhip_distortion_destroy(somhip_distortion *st) try {
  if (!st) return;
  if (somhip_engine *e = st->e) {                        // an orphan (engine destroyed first) has nothing left on the device
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    distortion_release(st);
    e->distortions.erase(std::remove(e->distortions.begin(), e->distortions.end(), st), e->distortions.end());
  }
  delete st;
} ABI_CATCH_VOID(somhip_distortion_destroy)
extern "C" int somhip_distortion_clear(somhip_distortion *st) try {
  CHK(check_distortion(st, true, "somhip_distortion_clear"));
  HIPCHK(hipSetDevice(st->e->device));
  CHK(distortion_zero(st));
  HIPCHK(hipStreamSynchronize(st->e->stream));
  return 0;
} ABI_CATCH(somhip_distortion_clear)

extern "C" int somhip_distortion_accumulate(somhip_distortion *st, somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n) try {
  const char *who = "somhip_distortion_accumulate";
  CHK(check_distortion(st, cb && ds, who));
  CHK(check_pair(cb, ds, who));
  CHK(distortion_check_codebook(st, cb, who));
  CHK(batchmap_check_data(ds, first, n, who));
  if (st->samples + (uint64_t)n >= (uint64_t)1 << 32)
    return fail("%s: %llu + %lld samples do not fit the 32-bit hit counts", who, (unsigned long long)st->samples, (long long)n);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  if (st->qs_cap < (size_t)n) {
    if (st->qs) HIPCHK(hipFree(st->qs));
    st->qs = nullptr; st->qs_cap = 0;
    HIPCHK(hipMalloc((void **)&st->qs, sizeof(double) * (size_t)n));
    st->qs_cap = (size_t)n;
  }
  BatchmapBufs b;
  CHK(batchmap_bind(cb, n, &b, st->S));
  CHK(batchmap_group_stage(cb, ds, first, n, b, nullptr, nullptr, KID_DISTORTION_GROUP));
  CHK(batchmap_sums_launch(cb, ds, first, b, true, KID_DISTORTION_SUMS));
  const int64_t waves = DS_THREADS / WAVE;                               // samples of a q workgroup, units of a q sums workgroup
  CHK(LAUNCH_TIMED(e, KID_DISTORTION_SUMS, k_distortion_q, dim3((unsigned)((n + waves - 1) / waves)), dim3(DS_THREADS), 0, ds->d_rows, ds->n, ds->d,
      first % ds->n, n, st->qs));
  CHK(LAUNCH_TIMED(e, KID_DISTORTION_SUMS, k_distortion_qsums, dim3((unsigned)((st->units + waves - 1) / waves)), dim3(DS_THREADS), 0,
      b.list, b.starts, (uint32_t)st->units, st->qs, st->Q));
  st->samples += (uint64_t)n;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_distortion_accumulate)

// The evaluate stage: e_j and the totals at radius r from the state's S and Q against the codebook's rows as they are.  It
// writes the state's evaluation room and the batch map's table scratch, nothing of the codebook.
static int distortion_evaluate_stage(somhip_distortion *st, somhip_codebook *cb, float r, double *unit_out, somhip_distortion_totals *totals) {
  somhip_engine *e = cb->e;
  const bool gauss = cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN;
  const int small_map = cb->v.xdim <= 1024 && cb->ydim <= 1024;         // (lattice_sq_small's condition)
  BatchmapBufs b;
  CHK(batchmap_bind(cb, 0, &b, st->S));
  const dim3 grid((unsigned)cb->v.ngroups, (unsigned)st->nblk);
  if (gauss) {
    const size_t t_len = batchmap_table_len(cb);
    CHK(LAUNCH_TIMED(e, KID_DISTORTION_EVALUATE, k_batchmap_gauss_table, dim3((unsigned)((t_len + BM_THREADS - 1) / BM_THREADS)), dim3(BM_THREADS), 0,
        cb->v.topol, cb->v.xdim, cb->ydim, r, b.table));
    CHK(LAUNCH_TIMED(e, KID_DISTORTION_EVALUATE, k_distortion_evaluate<true>, grid, dim3(256), 0, cb->v, cb->ydim, st->S, st->Q, r, small_map, b.table,
        st->pe, st->pm, st->da));
  } else {
    CHK(LAUNCH_TIMED(e, KID_DISTORTION_EVALUATE, k_distortion_evaluate<false>, grid, dim3(256), 0, cb->v, cb->ydim, st->S, st->Q, bubble_threshold(r),
        small_map, nullptr, st->pe, st->pm, st->da));
  }
  CHK(LAUNCH_TIMED(e, KID_DISTORTION_EVALUATE, k_distortion_units, dim3((unsigned)((st->units + DS_THREADS - 1) / DS_THREADS)), dim3(DS_THREADS), 0,
      st->pe, st->pm, st->da, (uint32_t)st->units, st->nblk, st->unit_e, st->unit_s));
  CHK(LAUNCH_TIMED(e, KID_DISTORTION_EVALUATE, k_distortion_fold, dim3(1), dim3(DS_FOLD_THREADS), 0, st->unit_e, st->unit_s, (uint32_t)st->units,
      st->totals));
  double t[2] = {0.0, 0.0};
  if (unit_out) CHK(to_host(e, unit_out, st->unit_e, (size_t)st->units));
  CHK(to_host_sync(e, t, st->totals, 2));
  totals->energy = t[0];
  totals->scale = t[1];
  totals->samples = st->samples;
  return 0;
}

extern "C" int somhip_distortion_evaluate(somhip_distortion *st, somhip_codebook *cb, float r, double *unit_out,
                                          somhip_distortion_totals *totals) try {
  const char *who = "somhip_distortion_evaluate";
  CHK(check_distortion(st, cb && totals, who));
  CHK(distortion_check_codebook(st, cb, who));
  if (!(r >= 0.0f)) return fail("%s: radius %g < 0", who, (double)r);
  HIPCHK(hipSetDevice(cb->e->device));
  return distortion_evaluate_stage(st, cb, r, unit_out, totals);
} ABI_CATCH(somhip_distortion_evaluate)

extern "C" int somhip_distortion_read(somhip_distortion *st, uint32_t *hits, double *sums, double *sq) try {
  CHK(check_distortion(st, true, "somhip_distortion_read"));
  somhip_engine *e = st->e;
  HIPCHK(hipSetDevice(e->device));
  const size_t units = (size_t)st->units, d = (size_t)st->d;
  std::vector<double> hs((hits || sums) ? units * (d + 1) : 0);
  if (sq) CHK(to_host(e, sq, st->Q, units));
  if (!hs.empty()) CHK(to_host(e, hs.data(), st->S, hs.size()));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (size_t u = 0; u < units && !hs.empty(); u++) {
    if (sums) memcpy(sums + u * d, hs.data() + u * (d + 1), sizeof(double) * d);
    if (hits) hits[u] = (uint32_t)hs[u * (d + 1) + d];                  // (an integer below 2^32, exact in fp64)
  }
  return 0;
} ABI_CATCH(somhip_distortion_read)

extern "C" int somhip_debug_distortion_evaluate(somhip_codebook *cb, float r, const uint32_t *hits, const double *sums, const double *sq,
                                                double *unit_out, somhip_distortion_totals *totals) try {
  const char *who = "somhip_debug_distortion_evaluate";
  CHK(check_codebook(cb, hits && sums && sq && totals, who));
  CHK(distortion_check_codebook(nullptr, cb, who));
  if (!(r >= 0.0f)) return fail("%s: radius %g < 0", who, (double)r);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  somhip_distortion *st = nullptr;
  CHK(distortion_new(cb, &st));
  auto run = [&]() -> int {
    const size_t units = (size_t)cb->v.n, d = (size_t)cb->v.d;
    std::vector<double> hs(units * (d + 1));
    for (size_t u = 0; u < units; u++) {
      memcpy(hs.data() + u * (d + 1), sums + u * d, sizeof(double) * d);
      hs[u * (d + 1) + d] = (double)hits[u];
      st->samples += hits[u];
    }
    CHK(to_device(e, st->S, hs.data(), hs.size()));
    CHK(to_device(e, st->Q, sq, units));
    return distortion_evaluate_stage(st, cb, r, unit_out, totals);      // (it waits for the stream: hs is read until then)
  };
  const int rc = run();
  somhip_distortion_destroy(st);
  return rc;
} ABI_CATCH(somhip_debug_distortion_evaluate)

// HIP-event totals of the distortion's stages since somhip_timing_reset, while somhip_timing_enable is on (ids of their own
// behind the published table): [0] group (winners pass, scan, sort), [1] the sums and the two Q passes, [2] evaluate (the
// gaussian table, the kernel, the two fold passes)
extern "C" int somhip_distortion_timing(somhip_engine *e, int64_t launches[3], double total_ms[3]) try {
  const int kid[3] = {KID_DISTORTION_GROUP, KID_DISTORTION_SUMS, KID_DISTORTION_EVALUATE};
  return stage_timing(e, "somhip_distortion_timing", kid, 3, launches, total_ms);
} ABI_CATCH(somhip_distortion_timing)
