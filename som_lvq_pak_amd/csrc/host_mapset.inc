// host_mapset.inc -- map sets: many maps of one shape on the device, trained at once with the reference's online algorithm
// (included by somhip.hip: one translation unit, shared static helpers; kernels/mapset.hpp)

// ---------------------------------------------------------------------------------
// the plan: pure host arithmetic (somhip_debug_mapset_plan)
// ---------------------------------------------------------------------------------
constexpr int64_t MAPSET_IMAGE_BUDGET = 128 * 1024;   // bytes of a map's LDS image, of the CU's 160 KiB
constexpr int MAPSET_CHUNK = 4096;                    // iterations per launch
constexpr int MAPSET_WINNER_SAMPLES = 64;             // samples per workgroup of k_mapset_winners
struct MapsetPlan { bool fits; int threads, upt, npad, dpad; int64_t image_bytes, lds_bytes; };
static MapsetPlan mapset_plan(int64_t n_rows, int dim) {
  MapsetPlan p{};
  const int64_t npad = (n_rows + WAVE - 1) / WAVE * WAVE;
  p.image_bytes = npad * (int64_t)dim * 4;
  p.fits = n_rows >= 1 && dim >= 1 && p.image_bytes <= MAPSET_IMAGE_BUDGET;
  if (!p.fits) return p;
  p.npad = (int)npad;
  p.threads = (int)std::min<int64_t>(npad, 64 * MAPSET_MAX_WAVES);
  p.upt = (int)((n_rows + p.threads - 1) / p.threads);
  p.dpad = (dim + 3) / 4 * 4;
  p.lds_bytes = MAPSET_RED_BYTES + p.image_bytes + 3 * (int64_t)p.dpad * 4 + 3 * (int64_t)p.dpad;
  // (a thread stages at most MAPSET_PF words of a sample: dim <= 32768 / npad <= 8 * 64 <= 8 * threads under the budget)
  if (dim > MAPSET_PF * p.threads) p.fits = false;
  return p;
}
extern "C" int somhip_debug_mapset_plan(int64_t n_rows, int dim, int masked, int32_t out[8]) try {
  if (!out) return fail("somhip_debug_mapset_plan: null output");
  if (n_rows < 1 || dim < 1) return fail("somhip_debug_mapset_plan: empty map (%lld x %d)", (long long)n_rows, dim);
  const MapsetPlan p = mapset_plan(n_rows, dim);
  const int32_t v[8] = {p.fits, p.threads, p.upt, (int32_t)p.lds_bytes, MAPSET_CHUNK, masked != 0, 0, 0};
  memcpy(out, v, sizeof v);
  return 0;
} ABI_CATCH(somhip_debug_mapset_plan)

// ---------------------------------------------------------------------------------
// the set
// ---------------------------------------------------------------------------------
struct somhip_mapset {
  somhip_engine *e = nullptr;
  float *d_rows = nullptr;          // [n_maps][n][d], row-major as the host has them
  int n_maps = 0;
  int64_t n = 0;
  int d = 0;
  MapLattice lat{};
  MapsetPlan plan{};
};
static MapsetShape mapset_shape(const somhip_mapset *ms) {
  return MapsetShape{(int)ms->n, ms->d, ms->plan.npad, ms->plan.upt, ms->plan.dpad, ms->lat.xdim, ms->lat.topol};
}
static void mapset_release(somhip_mapset *ms) {
  if (ms->d_rows) (void)hipFree(ms->d_rows);
  ms->d_rows = nullptr;
  ms->e = nullptr;
}
static int check_mapset(const somhip_mapset *ms, const char *who) {
  if (!ms) return fail("%s: null map set", who);
  if (!ms->e) return fail("%s: the engine of this map set was destroyed", who);
  return 0;
}
static int check_mapset_data(const somhip_mapset *ms, const somhip_dataset *ds, const char *who) {
  CHK(check_mapset(ms, who));
  if (!ds) return fail("%s: null data set", who);
  if (!ds->e) return fail("%s: the engine of this data set was destroyed", who);
  if (ds->e != ms->e) return fail("%s: map set and data belong to different engines", who);
  if (ds->d != ms->d) return fail("%s: map dimension (%d) != data dimension (%d)", who, ms->d, ds->d);
  return 0;
}
static int check_mapset_range(const somhip_mapset *ms, int first_map, int n_maps, const char *who) {
  if (first_map < 0 || n_maps < 0 || (int64_t)first_map + n_maps > ms->n_maps)
    return fail("%s: maps [%d,%lld) outside a set of %d", who, first_map, (long long)first_map + n_maps, ms->n_maps);
  return 0;
}

extern "C" int somhip_mapset_create(somhip_engine *e, const float *rows, int n_maps, int64_t n_rows, int dim, int topol, int neigh,
                                    int xdim, int ydim, somhip_mapset **out) try {
  if (!e || !rows || !out) return fail("somhip_mapset_create: null argument");
  if (n_maps < 1) return fail("somhip_mapset_create: %d maps", n_maps);
  if (topol != SOMHIP_TOPOL_HEXA && topol != SOMHIP_TOPOL_RECT) return fail("somhip_mapset_create: topology %d is not a map's (hexa, rect)", topol);
  if (neigh != SOMHIP_NEIGH_BUBBLE && neigh != SOMHIP_NEIGH_GAUSSIAN) return fail("somhip_mapset_create: can't set SOM parameters (neighbourhood %d)", neigh);
  if (n_rows <= 0 || dim <= 0) return fail("somhip_mapset_create: empty map (%lld x %d)", (long long)n_rows, dim);
  if (xdim <= 0 || ydim <= 0 || (int64_t)xdim * ydim != n_rows)
    return fail("somhip_mapset_create: map %dx%d does not have %lld units", xdim, ydim, (long long)n_rows);
  const MapsetPlan plan = mapset_plan(n_rows, dim);
  if (!plan.fits)
    return fail("somhip_mapset_create: the LDS image of a %lld x %d map is %lld bytes, the budget is %lld", (long long)n_rows, dim,
                (long long)plan.image_bytes, (long long)MAPSET_IMAGE_BUDGET);
  HIPCHK(hipSetDevice(e->device));
  somhip_mapset *ms = new somhip_mapset();
  ms->e = e; ms->n_maps = n_maps; ms->n = n_rows; ms->d = dim; ms->lat = MapLattice{topol, neigh, xdim, ydim}; ms->plan = plan;
  e->mapsets.push_back(ms);
  auto fill = [&]() -> int {
    const size_t bytes = sizeof(float) * (size_t)n_maps * (size_t)n_rows * dim;
    HIPCHK(hipMalloc((void **)&ms->d_rows, bytes));
    HIPCHK(hipMemcpy(ms->d_rows, rows, bytes, hipMemcpyHostToDevice));
    return 0;
  };
  if (int rc = fill()) { somhip_mapset_destroy(ms); return rc; }
  *out = ms;
  return 0;
} ABI_CATCH(somhip_mapset_create)
extern "C" void somhip_mapset_destroy(somhip_mapset *ms) try {
  if (!ms) return;
  if (somhip_engine *e = ms->e) {                        // an orphan (engine destroyed first) has nothing left on the device
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    mapset_release(ms);
    e->mapsets.erase(std::remove(e->mapsets.begin(), e->mapsets.end(), ms), e->mapsets.end());
  }
  delete ms;
} ABI_CATCH_VOID(somhip_mapset_destroy)
extern "C" int somhip_mapset_download(somhip_mapset *ms, int first_map, int n_maps, float *rows) try {
  CHK(check_mapset(ms, "somhip_mapset_download"));
  if (!rows) return fail("somhip_mapset_download: null argument");
  CHK(check_mapset_range(ms, first_map, n_maps, "somhip_mapset_download"));
  if (n_maps == 0) return 0;
  const size_t per = (size_t)ms->n * ms->d;
  HIPCHK(hipSetDevice(ms->e->device));
  CHK(to_host_sync(ms->e, rows, ms->d_rows + per * first_map, per * n_maps));
  return 0;
} ABI_CATCH(somhip_mapset_download)
extern "C" int somhip_mapset_upload(somhip_mapset *ms, int first_map, int n_maps, const float *rows) try {
  CHK(check_mapset(ms, "somhip_mapset_upload"));
  if (!rows) return fail("somhip_mapset_upload: null argument");
  CHK(check_mapset_range(ms, first_map, n_maps, "somhip_mapset_upload"));
  if (n_maps == 0) return 0;
  const size_t per = (size_t)ms->n * ms->d;
  HIPCHK(hipSetDevice(ms->e->device));
  CHK(to_device(ms->e, ms->d_rows + per * first_map, rows, per * n_maps));
  HIPCHK(hipStreamSynchronize(ms->e->stream));
  return 0;
} ABI_CATCH(somhip_mapset_upload)

// ---------------------------------------------------------------------------------
// som_training (som_rout.c:556-671), batch 1, for every map of the set at once
// ---------------------------------------------------------------------------------
// The run is cut into chunks of MAPSET_CHUNK iterations.  The scalars and the row indices of a chunk are made once, for
// all maps (they depend on the data row and the iteration only), in a pinned buffer of the engine's ring; one launch of
// k_mapset_train runs the chunk.  The host runs ahead of the GPU: it waits only where a ring buffer comes round again,
// or for the keys of a trace.
static int mapset_train(somhip_mapset *ms, somhip_dataset *ds, const somhip_som_params *p, int32_t *trace_index, float *trace_diff) {
  somhip_engine *e = ms->e;
  const bool G = ms->lat.neigh == SOMHIP_NEIGH_GAUSSIAN, M = ds->d_mask != nullptr, trace = trace_index || trace_diff;
  const int64_t CH = std::min<int64_t>(MAPSET_CHUNK, p->count);
  const MapsetShape shape = mapset_shape(ms);
  StepScalars *sc; int64_t *rowidx; uint64_t *keys = nullptr;
  CHK(scratch(e, SLOT_CALL_B, (size_t)CH, &sc));
  CHK(scratch(e, SLOT_PARTIAL, (size_t)CH, &rowidx));
  if (trace) CHK(scratch(e, SLOT_CALL_A, (size_t)CH * ms->n_maps, &keys));
  std::vector<uint64_t> hkeys(trace ? (size_t)CH * ms->n_maps : 0);
  for (int64_t off = 0; off < p->count; off += CH) {
    const int64_t c = std::min(CH, p->count - off);
    const int64_t it0 = p->start_iter + off, row0 = (p->data_first + off) % ds->n;
    void *pin; int slot;
    CHK(pin_acquire(e, (sizeof(StepScalars) + sizeof(int64_t)) * (size_t)c, &pin, &slot));
    StepScalars *hsc = (StepScalars *)pin;
    int64_t *hrow = (int64_t *)(hsc + c);
    CHK(som_scalars(ms->lat, ds, p, it0, c, row0, hsc));
    for (int64_t j = 0; j < c; j++) hrow[j] = (row0 + j) % ds->n;
    CHK(to_device(e, sc, hsc, (size_t)c));
    CHK(to_device(e, rowidx, hrow, (size_t)c));
    HIPCHK(hipEventRecord(e->pin_ev[slot], e->stream));
    {
      LaunchTimer t(e, KID_MAPSET_TRAIN);
      const int rc = with_value<1, 0>(G, [&](auto g) { return with_value<1, 0>(M, [&](auto m) {
        constexpr bool GG = decltype(g)::value != 0, MM = decltype(m)::value != 0;
        CHK(raise_lds_limit(e, (LdsKernel)(LDS_MAPSET_TRAIN + 2 * GG + MM), (const void *)(k_mapset_train<GG, MM>), MAPSET_LDS_LIMIT));
        return LAUNCH(e, (k_mapset_train<GG, MM>), dim3((unsigned)ms->n_maps), dim3((unsigned)ms->plan.threads), (size_t)ms->plan.lds_bytes, shape,
                      ms->d_rows, ds->d_rows, ds->d_mask, sc, rowidx, (int)c, keys);
      }); });
      CHK(rc);
    }
    if (trace) {
      CHK(to_host_sync(e, hkeys.data(), keys, (size_t)c * ms->n_maps));   // (hsc is still this chunk's: the ring has not come round)
      for (int m = 0; m < ms->n_maps; m++)
        som_trace(hsc, hkeys.data() + (size_t)m * c, c, (int64_t)m * p->count + off, trace_index, trace_diff);
    }
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}
extern "C" int somhip_mapset_train(somhip_mapset *ms, somhip_dataset *ds, const somhip_som_params *p, int32_t *trace_index,
                                   float *trace_diff) try {
  CHK(check_mapset_data(ms, ds, "somhip_mapset_train"));
  if (!p) return fail("somhip_mapset_train: null params");
  if (p->batch != 1) return fail("somhip_mapset_train: batch %lld -- a map set trains with the online schedule only (batch 1)", (long long)p->batch);
  if (p->length <= 0 || p->count < 0 || p->start_iter < 0 || p->start_iter + p->count > p->length || p->data_first < 0)
    return fail("somhip_mapset_train: iterations [%lld,%lld) outside schedule of %lld",
                (long long)p->start_iter, (long long)(p->start_iter + p->count), (long long)p->length);
  if (p->count == 0) return 0;
  HIPCHK(hipSetDevice(ms->e->device));
  return mapset_train(ms, ds, p, trace_index, trace_diff);
} ABI_CATCH(somhip_mapset_train)

// find_winner_euc of data rows [first, first + count) against every map of the set
extern "C" int somhip_mapset_winners(somhip_mapset *ms, somhip_dataset *ds, int64_t first, int64_t count, int32_t *index,
                                     float *diff, int32_t *ret) try {
  CHK(check_mapset_data(ms, ds, "somhip_mapset_winners"));
  if (!index || !diff) return fail("somhip_mapset_winners: null output");
  if (first < 0) return fail("somhip_mapset_winners: first row %lld < 0", (long long)first);
  if (count <= 0) return 0;
  somhip_engine *e = ms->e;
  HIPCHK(hipSetDevice(e->device));
  const bool M = ds->d_mask != nullptr;
  const MapsetShape shape = mapset_shape(ms);
  // a run is cut so that its keys stay below 64 MiB
  const int64_t CH = std::max<int64_t>(MAPSET_WINNER_SAMPLES, std::min<int64_t>(count, (8ll << 20) / ms->n_maps));
  uint64_t *keys;
  CHK(scratch(e, SLOT_CALL_A, (size_t)std::min(CH, count) * ms->n_maps, &keys));
  std::vector<uint64_t> hk((size_t)std::min(CH, count) * ms->n_maps);
  for (int64_t off = 0; off < count; off += CH) {
    const int64_t c = std::min(CH, count - off), f = (first + off) % ds->n;
    {
      LaunchTimer t(e, KID_MAPSET_WINNERS);
      const int rc = with_value<1, 0>(M, [&](auto m) {
        constexpr bool MM = decltype(m)::value != 0;
        CHK(raise_lds_limit(e, (LdsKernel)(LDS_MAPSET_WINNERS + MM), (const void *)(k_mapset_winners<MM>), MAPSET_LDS_LIMIT));
        return LAUNCH(e, (k_mapset_winners<MM>), dim3((unsigned)ms->n_maps, (unsigned)((c + MAPSET_WINNER_SAMPLES - 1) / MAPSET_WINNER_SAMPLES)),
                      dim3((unsigned)ms->plan.threads), (size_t)ms->plan.lds_bytes, shape, ms->d_rows, ds->d_rows, ds->d_mask, ds->n, f, c,
                      MAPSET_WINNER_SAMPLES, keys);
      });
      CHK(rc);
    }
    CHK(to_host_sync(e, hk.data(), keys, (size_t)c * ms->n_maps));
    for (int64_t i = 0; i < c; i++) {
      const bool empty = sample_is_empty(ds, (f + i) % ds->n);
      for (int m = 0; m < ms->n_maps; m++) {
        const size_t o = (size_t)m * count + off + i;
        if (empty) { index[o] = -2; diff[o] = -1.0f; }
        else decode_key(hk[(size_t)m * c + i], false, &index[o], &diff[o]);
        if (ret) ret[o] = empty ? 0 : 1;
      }
    }
  }
  return 0;
} ABI_CATCH(somhip_mapset_winners)

// HIP-event totals of the two set kernels since somhip_timing_reset, while somhip_timing_enable is on (the kernel table
// of somhip_kernel_count is closed; these two are timed under ids of their own): [0] k_mapset_train, [1] k_mapset_winners
extern "C" int somhip_mapset_timing(somhip_engine *e, int64_t launches[2], double total_ms[2]) try {
  const int kid[2] = {KID_MAPSET_TRAIN, KID_MAPSET_WINNERS};
  return stage_timing(e, "somhip_mapset_timing", kid, 2, launches, total_ms);
} ABI_CATCH(somhip_mapset_timing)
