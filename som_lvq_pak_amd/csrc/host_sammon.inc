// host_sammon.inc -- Sammon mapping of a codebook (kernels/sammon.hpp): zero-distance pairs and the iteration
// (part of somhip.hip: same translation unit)

// the distance table of n rows: a full symmetric fp32 matrix, rows padded to whole waves
struct SammonTable {
  int64_t ld;
  size_t bytes;
};
static SammonTable sammon_table(int64_t noc) {
  SammonTable t;
  t.ld = (noc + WAVE - 1) / WAVE * WAVE;
  t.bytes = sizeof(float) * (size_t)noc * (size_t)t.ld;
  return t;
}

static int sammon_check_codebook(const char *who, somhip_codebook *cb) {
  if (!cb) return fail("%s: null codebook", who);
  if (!cb->e) return fail("%s: the engine of this codebook was destroyed", who);
  if (is_shard(cb))
    return fail("%s: the codebook is a shard (%lld of %lld rows); the Sammon mapping needs the whole one", who,
                (long long)cb->v.n, (long long)cb->n_global);
  if (cb->v.n > (int64_t)SAMMON_TILE * 65535)             // the pair tiles are a two-dimensional grid
    return fail("%s: %lld rows are more than this path indexes", who, (long long)cb->v.n);
  return 0;
}

// the rows in unit order, row-major, in SLOT_STAGE
static int sammon_stage_rows(somhip_codebook *cb, const float **rows) {
  somhip_engine *e = cb->e;
  float *stage;
  CHK(scratch(e, SLOT_STAGE, (size_t)cb->v.n * cb->v.d, &stage));
  CHK(LAUNCH_TIMED(e, KID_LAYOUT, k_tiles_to_rows, dim3((unsigned)cb->v.ngroups), dim3(256), 0, stage, cb->v));
  *rows = stage;
  return 0;
}

// the one launch site of k_sammon_dist: table and / or zero pairs; *n_zero (host) = number of pairs with dd == 0
static int sammon_distances(somhip_codebook *cb, const float *rows, float *D, int64_t ld, uint32_t *d_pairs, int64_t cap,
                            unsigned long long *n_zero) {
  somhip_engine *e = cb->e;
  unsigned long long *d_count;
  CHK(scratch(e, SLOT_CALL_A, 1, &d_count));
  HIPCHK(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), e->stream));
  const unsigned tiles = (unsigned)((cb->v.n + SAMMON_TILE - 1) / SAMMON_TILE);
  CHK(LAUNCH_TIMED(e, KID_SAMMON_DIST, k_sammon_dist, dim3(tiles, tiles), dim3(256), 0, rows, (int)cb->v.n, cb->v.d, D, ld, d_pairs,
      (unsigned long long)cap, d_count));
  return to_host_sync(e, n_zero, d_count, 1);
}

extern "C" int somhip_sammon_zero_pairs(somhip_codebook *cb, uint32_t *pairs, int64_t cap, int64_t *n_pairs) try {
  CHK(sammon_check_codebook("somhip_sammon_zero_pairs", cb));
  if (!n_pairs || cap < 0 || (cap > 0 && !pairs)) return fail("somhip_sammon_zero_pairs: bad arguments");
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  if (!pairs) cap = 0;
  const float *rows;
  CHK(sammon_stage_rows(cb, &rows));
  uint32_t *d_pairs = nullptr;
  if (cap > 0) CHK(scratch(e, SLOT_PAIRS, 2 * (size_t)cap, &d_pairs));
  unsigned long long found = 0;
  CHK(sammon_distances(cb, rows, nullptr, 0, d_pairs, cap, &found));
  *n_pairs = (int64_t)found;
  const int64_t have = std::min<int64_t>((int64_t)found, cap);
  if (have > 0) {
    CHK(to_host_sync(e, pairs, d_pairs, 2 * (size_t)have));
    std::vector<uint64_t> keys((size_t)have);                  // sort by (i, j): the kernel appends in no order
    for (int64_t t = 0; t < have; t++) keys[(size_t)t] = ((uint64_t)pairs[2 * t] << 32) | pairs[2 * t + 1];
    std::sort(keys.begin(), keys.end());
    for (int64_t t = 0; t < have; t++) { pairs[2 * t] = (uint32_t)(keys[(size_t)t] >> 32); pairs[2 * t + 1] = (uint32_t)keys[(size_t)t]; }
  }
  return 0;
} ABI_CATCH(somhip_sammon_zero_pairs)

// device memory of one somhip_sammon call; freed on every way out
struct SammonBufs {
  float *D = nullptr, *xy = nullptr;          // xy: x, y, xu, yu, each ld long
  double *part = nullptr;
  ~SammonBufs() {
    if (D) (void)hipFree(D);
    if (xy) (void)hipFree(xy);
    if (part) (void)hipFree(part);
  }
};

extern "C" int somhip_sammon(somhip_codebook *cb, int64_t rlen, float *x, float *y, double *mapping_error) try {
  CHK(sammon_check_codebook("somhip_sammon", cb));
  if (!x || !y || rlen < 0) return fail("somhip_sammon: bad arguments");
  if (cb->v.n < 2) return fail("somhip_sammon: a codebook of %lld row(s) has no pair to map", (long long)cb->v.n);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const int noc = (int)cb->v.n;
  const SammonTable pl = sammon_table(noc);
  SammonBufs b;
  if (hipMalloc((void **)&b.D, pl.bytes) != hipSuccess) {
    (void)hipGetLastError();
    b.D = nullptr;
    return fail("somhip_sammon: cannot allocate the %d x %lld distance table (%.2f GB of device memory)", noc,
                (long long)pl.ld, (double)pl.bytes / 1e9);
  }
  HIPCHK(hipMalloc((void **)&b.xy, sizeof(float) * 4 * (size_t)pl.ld));
  float *dx = b.xy, *dy = b.xy + pl.ld, *dxu = b.xy + 2 * pl.ld, *dyu = b.xy + 3 * pl.ld;
  const unsigned err_blocks = (unsigned)std::min<int>(noc - 1, 2048);
  std::vector<double> part;
  if (mapping_error) {
    HIPCHK(hipMalloc((void **)&b.part, sizeof(double) * 2 * err_blocks));
    part.resize(2 * (size_t)err_blocks);
  }
  const float *rows;
  CHK(sammon_stage_rows(cb, &rows));
  unsigned long long n_zero = 0;
  CHK(sammon_distances(cb, rows, b.D, pl.ld, nullptr, 0, &n_zero));
  if (n_zero) return fail("somhip_sammon: %llu pair(s) of rows at distance 0 (somhip_sammon_zero_pairs lists them): the "
                          "iteration would divide by it -- remove the identical rows first", n_zero);
  CHK(to_device(e, dx, x, (size_t)noc));
  CHK(to_device(e, dy, y, (size_t)noc));
  for (int64_t it = 0; it < rlen; it++) {
    CHK(LAUNCH_TIMED(e, KID_SAMMON_SWEEP, k_sammon_sweep, dim3((unsigned)((noc + SAMMON_JB - 1) / SAMMON_JB)), dim3(256), 0, b.D, pl.ld, noc, dx, dy,
        dxu, dyu));
    CHK(LAUNCH_TIMED(e, KID_SAMMON_CENTRE, k_sammon_centre, dim3(1), dim3(256), 0, dxu, dyu, dx, dy, noc));
    if (mapping_error) {
      CHK(LAUNCH_TIMED(e, KID_SAMMON_ERROR, k_sammon_error, dim3(err_blocks), dim3(256), 0, b.D, pl.ld, noc, dx, dy, b.part));
      CHK(to_host_sync(e, part.data(), b.part, part.size()));
      double es = 0.0, tot = 0.0;
      for (unsigned k = 0; k < err_blocks; k++) { es += part[2 * k]; tot += part[2 * k + 1]; }
      mapping_error[it] = es / tot;
    }
  }
  CHK(to_host(e, x, dx, (size_t)noc));
  CHK(to_host_sync(e, y, dy, (size_t)noc));
  return 0;
} ABI_CATCH(somhip_sammon)
