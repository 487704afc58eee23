// host_som.inc -- som_training: per-iteration scalars, online (graph-replayed) and mini-batch drivers
// (included by somhip.hip: one translation unit, shared static helpers)

// ---------------------------------------------------------------------------------
// som_training
// ---------------------------------------------------------------------------------
// Bubble threshold for maps with both sides <= 1024: every squared lattice distance is then an exact
// multiple of 1/4, so only K = floor(4 T) matters (T = bubble_threshold(radius)) and K/4 is an
// equivalent threshold.  K is constant while the radius stays inside [f(K/4), f((K+1)/4)), f(r) =
// (float)sqrt((double)r) -- the schedule moves the radius by ~1e-4 per iteration, so the exact
// search runs only when a lattice distance is crossed.
struct ThreshCache {
  bool valid = false;
  float lo = 0.f, hi = 0.f, thresh = -1.f;
  float get(float radius) {
    if (!(radius >= 0.0f)) return -1.0f;
    if (valid && radius >= lo && radius < hi) return thresh;
    const float T = bubble_threshold(radius);
    const double k = std::floor(4.0 * (double)T);
    thresh = (float)(k / 4.0);
    lo = (float)std::sqrt(k / 4.0);
    hi = (float)std::sqrt((k + 1.0) / 4.0);
    valid = hi > lo;
    return thresh;
  }
};

// what the scalars need to know of the map: a codebook's lattice, or a map set's
struct MapLattice { int topol, neigh, xdim, ydim; };
static MapLattice lattice_of(const somhip_codebook *cb) { return MapLattice{cb->v.topol, cb->v.neigh, cb->v.xdim, cb->ydim}; }
static int som_scalars(const MapLattice &lat, const somhip_dataset *ds, const somhip_som_params *p,
                       int64_t it0, int64_t cnt, int64_t row0, StepScalars *out) {
  const bool gauss = lat.neigh == SOMHIP_NEIGH_GAUSSIAN;
  const bool small_map = lat.xdim <= 1024 && lat.ydim <= 1024;
  ThreshCache tc;
  for (int64_t j = 0; j < cnt; j++) {
    int64_t le = it0 + j, r = (row0 + j) % ds->n;
    float trad = radius_at(le, p->length, p->radius);
    float talp = alpha_at(p->alpha_type, le, p->length, p->alpha);
    float w = ds->weight.empty() ? 0.0f : (float)ds->weight[(size_t)r];
    if (w > 0.0f && p->use_weights) talp = weighted_alpha(talp, w);
    StepScalars s;
    s.alpha = talp;
    s.thresh = gauss ? trad : (small_map ? tc.get(trad) : bubble_threshold(trad));
    s.fixed = -1;
    // lattice rows a neighbourhood of this radius can span: hexa rows are sqrt(0.75)
    // apart (som_rout.c:451), rect rows 1 apart; +1 keeps it conservative
    double reach = gauss ? 1e9 : (trad > 0.0f ? (double)trad / (lat.topol == SOMHIP_TOPOL_RECT ? 1.0 : 0.8660254037844386) + 1.0 : 1.0);
    s.reach = reach > 1e6 ? 1000000 : (int32_t)reach;
    if (sample_is_empty(ds, r)) s.reach = -1;
    if (p->use_fixed && !ds->fixed_xy.empty() && ds->fixed_xy[(size_t)(2 * r)] >= 0) {
      int fx = ds->fixed_xy[(size_t)(2 * r)], fy = ds->fixed_xy[(size_t)(2 * r + 1)];
      // the reference hands xfix / yfix to the neighbourhood function as they are (som_rout.c:628-632), also when
      // they lie beyond the map's edge: the scalars carry the lattice coordinates themselves (non-negative ones:
      // somhip_dataset_create keeps a negative coordinate to mean "no fixed point")
      s.fixed = fixed_pack(fx, fy);
      if (s.reach < 0) s.reach = reach > 1e6 ? 1000000 : (int32_t)reach;
    }
    out[j] = s;
  }
  return 0;
}

constexpr int ONLINE_U = 8;    // chunks (KiB) per register buffer; two buffers per wave
static int launch_online_any(somhip_engine *e, const somhip_codebook *cb, const somhip_dataset *ds, bool G, bool M,
                              const int64_t *prev_row, const int64_t *cur_row, int has_prev, int has_cur, const uint64_t *prev_slot,
                              uint64_t *cur_slot, const StepScalars *prev_sc, const StepScalars *cur_sc) {
  // chunks (KiB) per register buffer: a wave is alone on its SIMD here (one wave per 64 rows: 1024 waves on 1024 SIMDs at
  // 65536 rows), so registers are free and what bounds the kernel is how many bytes it keeps in flight
  return with_value<1, 0>(G, [&](auto g) { return with_value<1, 0>(M, [&](auto m) {
    constexpr bool GG = decltype(g)::value != 0, MM = decltype(m)::value != 0;
    return LAUNCH_TIMED(e, KID_SOM_ONLINE_STEP, (k_som_online_step<GG, MM, ONLINE_U>), dim3((unsigned)((cb->v.ngroups + 3) / 4)), dim3(256), 0, cb->v,
                        ds->d_rows, ds->d_mask, prev_row, cur_row, has_prev, has_cur, prev_slot, cur_slot, prev_sc, cur_sc);
  }); });
}
// the winner trace of iterations [off, off + c): a fixed point (-3, -1), a skipped sample (-2, -1), else the key's row and distance
static void som_trace(const StepScalars *sc, const uint64_t *keys, int64_t c, int64_t off, int32_t *trace_index, float *trace_diff) {
  for (int64_t j = 0; j < c; j++) {
    int32_t idx; float df;
    if (sc[j].fixed >= 0) { idx = -3; df = -1.0f; }
    else if (sc[j].reach < 0) { idx = -2; df = -1.0f; }
    else decode_key(keys[j], false, &idx, &df);
    if (trace_index) trace_index[off + j] = idx;
    if (trace_diff) trace_diff[off + j] = df;
  }
}

// The online algorithm is one small launch per iteration; a full chunk of them is captured
// once into a hipGraph (all per-iteration inputs live in device arrays the host refreshes) and
// replayed, which removes the per-launch host cost that bounds small maps.
static int som_train_online(somhip_codebook *cb, somhip_dataset *ds, const somhip_som_params *p,
                            int32_t *trace_index, float *trace_diff) {
  somhip_engine *e = cb->e;
  rows_written(cb);
  const int64_t CH = ONLINE_CHUNK;
  const bool G = cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN, M = ds->d_mask != nullptr;
  uint64_t *slot; StepScalars *sc; int64_t *rowidx;
  // entry 0 of the arrays carries the last iteration of the previous chunk
  CHK(scratch(e, SLOT_CALL_A, (size_t)(CH + 1), &slot));
  CHK(scratch(e, SLOT_CALL_B, (size_t)(CH + 1), &sc));
  CHK(scratch(e, SLOT_PARTIAL, (size_t)(CH + 1), &rowidx));
  std::vector<StepScalars> hsc((size_t)CH + 1);
  std::vector<uint64_t> hslot((size_t)CH + 1);
  std::vector<int64_t> hrow((size_t)CH + 1);
  // entry 0 before the first iteration: "teaches nothing" (reach < 0), so has_prev can always be 1
  hsc[0].alpha = 0.f; hsc[0].thresh = -1.f; hsc[0].fixed = -1; hsc[0].reach = -1;
  hrow[0] = 0;
  CHK(to_device(e, sc, hsc.data(), 1));
  CHK(to_device(e, rowidx, hrow.data(), 1));
  HIPCHK(hipMemsetAsync(slot, 0xFF, sizeof(uint64_t), e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));

  // graph of one full chunk, cached per engine while its arguments stay the same
  OnlineGraphKey key{cb->v.tiles, cb->v.n, cb->v.d, cb->v.patch_w, cb->v.row_offset, cb->v.xdim, cb->v.topol,
                     ds->d_rows, ds->d_mask, slot, sc, rowidx, G, M};
  const bool want_graph = !e->timing && p->count >= CH;
  if (want_graph && !(e->online_graph_exec && e->online_graph_key == key)) {
    if (e->online_graph_exec) { (void)hipGraphExecDestroy(e->online_graph_exec); e->online_graph_exec = nullptr; }
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal));
    int launch_rc = 0;
    for (int64_t j = 0; j < CH && !launch_rc; j++)
      launch_rc = launch_online_any(e, cb, ds, G, M, rowidx + j, rowidx + j + 1, 1, 1, slot + j, slot + j + 1, sc + j, sc + j + 1);
    // the capture is always ended -- a stream left capturing would fail every later call on this engine
    const hipError_t end_err = hipStreamEndCapture(e->stream, &graph);
    if (launch_rc || end_err != hipSuccess) {
      if (graph) (void)hipGraphDestroy(graph);
      return launch_rc ? launch_rc : fail("som_training: capturing the online chunk failed: %s", hipGetErrorString(end_err));
    }
    const hipError_t inst_err = hipGraphInstantiate(&e->online_graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (inst_err != hipSuccess) { e->online_graph_exec = nullptr; return fail("som_training: hipGraphInstantiate: %s", hipGetErrorString(inst_err)); }
    e->online_graph_key = key;
  }

  bool have_prev = false;
  for (int64_t off = 0; off < p->count; off += CH) {
    int64_t c = std::min(CH, p->count - off);
    int64_t it0 = p->start_iter + off, row0 = (p->data_first + off) % ds->n;
    CHK(som_scalars(lattice_of(cb), ds, p, it0, c, row0, hsc.data() + 1));
    for (int64_t j = 0; j < c; j++) hrow[(size_t)j + 1] = (row0 + j) % ds->n;
    CHK(to_device(e, sc + 1, hsc.data() + 1, (size_t)c));
    CHK(to_device(e, rowidx + 1, hrow.data() + 1, (size_t)c));
    HIPCHK(hipMemsetAsync(slot + 1, 0xFF, sizeof(uint64_t) * (size_t)c, e->stream));
    if (want_graph && c == CH) {
      HIPCHK(hipGraphLaunch(e->online_graph_exec, e->stream));
    } else {
      for (int64_t j = 0; j < c; j++)
        CHK(launch_online_any(e, cb, ds, G, M, rowidx + j, rowidx + j + 1, 1, 1, slot + j, slot + j + 1, sc + j, sc + j + 1));
    }
    have_prev = true;
    if (trace_index || trace_diff) {
      CHK(to_host_sync(e, hslot.data(), slot + 1, (size_t)c));
      som_trace(hsc.data() + 1, hslot.data(), c, off, trace_index, trace_diff);
    }
    // carry the last iteration's slot + scalars + row into entry 0 for the next chunk / the flush
    CHK(on_device(e, slot, slot + c, 1));
    CHK(on_device(e, sc, sc + c, 1));
    CHK(on_device(e, rowidx, rowidx + c, 1));
    // the host staging vectors are reused by the next chunk
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if (have_prev)   // flush: apply the last iteration's update
    CHK(launch_online_any(e, cb, ds, G, M, rowidx, rowidx, 1, 0, slot, slot, sc, sc));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// diagnostics (include/somhip.h): the device addresses the cached graph's key compares, for the tests that train a
// second codebook or data set on an engine that holds a graph
extern "C" int somhip_debug_device_ptrs(somhip_codebook *cb, somhip_dataset *ds, uint64_t *out) try {
  CHK(check_pair(cb, ds, "somhip_debug_device_ptrs"));
  if (!out) return fail("somhip_debug_device_ptrs: null argument");
  out[0] = (uint64_t)(uintptr_t)cb->v.tiles; out[1] = (uint64_t)(uintptr_t)ds->d_rows; out[2] = (uint64_t)(uintptr_t)ds->d_mask;
  return 0;
} ABI_CATCH(somhip_debug_device_ptrs)

// The mini-batch update of one run: som_update_plan makes every choice, the stages only read it -- decode (K4a) ->
// members (K4b) -> order (K4c) -> apply.  K4b writes its entries for the apply kernel the plan picks: what an entry
// carries (`entry`), its mask field holding packed winner coordinates (`gauss_gemm`) and only a list's tail (`tail`).
enum UpdateApply { APPLY_GEMM, APPLY_GAUSS_H, APPLY_GAUSS_S, APPLY_BUBBLE_S, APPLY_RUN };
enum UpdateEntry { ENTRY_SAMPLE, ENTRY_FLOAT4, ENTRY_BYTE };   // sample index in the run, row offset in float4s, in bytes
struct UpdatePlan {
  UpdateApply apply; UpdateEntry entry;
  int qw = 0, ntw = 0;      // bubble_s / run: chunks (float4) per wave (2, 4); gemm: 32-dim tiles per wave (1, 2, 4)
  bool off32 = false;       // bubble_s: byte offsets in the entries and register-offset scalar loads (OFF32)
  bool decode;              // k_decode_winners runs and K4b reads its coordinates (else K4b decodes the keys itself)
  int members_nt, members_rr;   // K4b's threads per workgroup (256, 1024) and samples per thread and trip (4, 8)
  bool gauss_gemm;          // the entries carry the winner's packed coordinates for the gaussian gemm form
  bool tail;                // gemm, bubble: K4b says where each list starts (lstart) and makes only its tail ...
  uint32_t tail_need = 0;   // ... until it holds this many entries with every live unit (0: the whole list)
  int reach_max = -1;       // decoded winners, bubble: the run's largest reach (K4b's early rejection), else -1
  bool order;               // k_order_groups runs (the apply kernels take the groups in its order)
  dim3 grid, block;         // the apply kernel's launch
};

static UpdatePlan som_update_plan(const somhip_codebook *cb, const somhip_dataset *ds, int64_t data_first, int64_t count,
                                  const StepScalars *h_sc) {
  const bool G = cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN, M = ds->d_mask != nullptr;
  UpdatePlan p;
  // chunks (float4) per wave (4 waves of a workgroup share a member list): more chunks amortise the per-entry
  // work, fewer give more waves -- a small shard (N > 1 ranks) needs them to keep the vector ALUs busy.  Measured
  // (profiles/r01_shard_rehearsal.txt): 4 with the pipelined tile walk beats 8 even on the whole 65536-row map.
  int QW = 4;
  while (QW > 2 && (int64_t)cb->v.ngroups * ((cb->v.d4 + QW - 1) / QW) < 8192) QW >>= 1;
  if (const char *s = getenv("SOMHIP_UPD_QW")) { const int v = atoi(s); if (v == 2 || v == 4) QW = v; }
  // bubble, no masks, whole chunks, enough waves at 4 chunks each: the scalar-operand kernel K4s (a shard so small
  // that QW fell to 2 is better off with K4's pipelined tile walk); K4b then writes row offsets into the entries
  // data sets below 4 GiB: byte offsets in the entries and register-offset scalar loads (OFF32)
  const bool off32_ok = ds->n * (int64_t)cb->v.d * 4 < (1ll << 32);
  // 2 chunks per wave (a small shard) only with OFF32: with ten scalar instructions of address work per entry the
  // scalar unit, not the 12 packed vector instructions, was the bound (8 shards of the 256x256x512 map: 225 -> 203 us;
  // the LDS-tile kernel: 241)
  const bool scalar_form = !G && !M && (QW == 4 || (QW == 2 && off32_ok)) && (cb->v.d & 3) == 0 && cb->v.d4 % (4 * QW) == 0 &&
                           count <= ds->n && ds->n * (int64_t)(cb->v.d >> 2) < (1ll << 32) && !getenv("SOMHIP_UPD_LDS");
  // the matrix-pipe form of the same update (kernels/som_update_gemm.hpp): opt-in, bubble, no masks, dims in whole 128s
  // (gaussian: lattice_sq in fp32 needs both map sides <= 1024, the winner's coordinates travel as 10-bit fields)
  bool gemm_form = cb->e->update_mode == SOMHIP_UPDATE_GEMM && !M && cb->v.d % 128 == 0 && count <= GEMM_MAX_RUN &&
                   ds->n * (int64_t)(cb->v.d >> 2) < (1ll << 32) &&      // the entries carry 32-bit row offsets in float4 units
                   (!G || (cb->v.xdim <= 1024 && cb->ydim <= 1024));
  // one pass over the run's scalars: the smallest rate (for the list tail below), and what the GEMM form cannot take --
  // a rate outside [0, 1] (the backward walk's decay P (1 - a) would change sign and stop it early; NaN fails the test
  // too), or, gaussian, a fixed point with a coordinate above 1023 (it would not fit the entry's 10-bit fields)
  float amin = 1.0f;
  for (int64_t j = 0; j < count && gemm_form; j++) {
    const StepScalars &s = h_sc[j];
    if (!(s.alpha >= 0.0f && s.alpha <= 1.0f) || (G && s.fixed >= 0 && (fixed_x(s.fixed) > 1023 || fixed_y(s.fixed) > 1023))) gemm_form = false;
    amin = std::min(amin, s.alpha);
  }
  p.off32 = scalar_form && off32_ok && !gemm_form;
  p.entry = p.off32 ? ENTRY_BYTE : scalar_form || gemm_form ? ENTRY_FLOAT4 : ENTRY_SAMPLE;
  p.gauss_gemm = G && gemm_form;
  // the winners' lattice coordinates: K4b decodes them itself from the keys (a division per (sample, row group), but no
  // launch) in a short run; a long run pays for the launch many times over (1024 groups x 32768 samples: members 201 -> 180 us, the decode launch 6)
  // ... and from 8192 samples on where the map has 512 row groups and more: the 4 us of the launch are paid back per group
  // (1024 groups x 8192 samples at radius 20 -> 1: members 121 -> 42 us with the two-phase form in one trip of 1024 x 8)
  p.decode = G || count >= 16384 || (count >= 8192 && cb->v.ngroups >= 512);   // (the gaussian update needs the decoded winners itself)
  // the GEMM update walks a list from its end and stops once every unit's decay is below GEMM_CUT: K4b then makes only
  // the tail that walk can reach -- until it holds `tail_need` entries with every live unit in them: (1 - a_min)^need <
  // GEMM_CUT for the smallest rate a_min of the run, + one chunk so that the walk's last, whole chunk is there too
  p.tail = gemm_form && !G && !getenv("SOMHIP_GEMM_FULL_LISTS");
  if (p.tail && amin > 1e-6f && amin < 1.0f) {
    const double need = std::ceil(std::log((double)GEMM_CUT) / std::log1p(-(double)amin)) + GEMM_KT + 1;
    if (need < (double)count / 2) p.tail_need = (uint32_t)need;
  }
  // (see k_som_members: early rejection on the winners' coordinates)
  if (p.decode && !G) { for (int64_t j = 0; j < count; j++) p.reach_max = std::max(p.reach_max, (int)h_sc[j].reach); }
  // a small shard has few row groups: 1024 threads each (one trip over a 4096 batch) instead of 256
  bool wide = cb->v.ngroups < 512 && count > 1024;
  // ... and so does a long run whose lists will not be cut short: a trip costs two barriers and a scan whatever it
  // finds, and with a small neighbourhood it finds a handful of members per 1024 samples (step_probe.py: 0.47 ms per
  // 32768 vectors at radius 20-33 in trips of 1024, against 0.06 ms at radius 128 where the tail is full after one trip).
  // Trips of 1024 only while the tail the GEMM update needs is expected within three of them: the share of the samples
  // whose neighbourhood covers a whole 8 x 8 patch is about area(radius - 6) / units.
  if (!wide && !G && count >= 8192) {
    const double r = std::sqrt((double)std::max(h_sc[count - 1].thresh, 0.0f)) - 6.0;
    const double full = r > 0.0 ? std::min(1.0, 3.6276 * r * r / std::max<double>(1.0, (double)cb->v.xdim * cb->ydim)) : 0.0;
    wide = p.tail_need == 0 || (double)p.tail_need > 3.0 * 1024.0 * full;
  }
  p.members_nt = wide ? 1024 : 256;
  // (decoded winners, long run, lists not cut short: 8 samples per thread -- four trips over a 32768-vector run, one over 8192; what a
  // trip costs besides the membership arithmetic of the queued samples is its barriers and dependent loads)
  p.members_rr = wide && !G && p.decode && p.reach_max >= 0 && count >= 8192 ? 8 : 4;
  p.order = cb->v.ngroups <= 8192;                        // (k_order_groups holds the counts in LDS)
  if (gemm_form) {
    p.apply = APPLY_GEMM;
    // dims per workgroup: 256 when the lists are long, 128 when they are short -- a workgroup is then mostly its fixed
    // costs, and more of them run side by side -- or when a small shard would not fill the chip.  Expected entries per
    // list: the run's samples x the share of the map a neighbourhood (dilated by a row group's 8x8 patch) covers.
    // (Round 3: 512-dim workgroups -- 64 KiB of LDS, two per CU -- kept the matrix pipe busy 46 % of the time, the rest
    // was spent waiting for the next chunk's rows; at 256 dims four fit and the kernel is 4-20 % faster at every
    // radius of the configs[3] schedule, profiles/r03_gemm_ntw.txt.)
    p.ntw = G && cb->v.d % 512 == 0 ? 4 : cb->v.d % 256 == 0 ? 2 : 1;    // (gaussian: the rates are made once per workgroup slice -- wide)
    const float r = sqrtf(std::max(h_sc[0].thresh, 0.0f)) + 4.5f;
    const double expect = (double)count * 3.14159265 * r * r / std::max<double>(1.0, (double)cb->v.xdim * cb->ydim);
    const int by_len = G ? 4 : expect < 64.0 ? 1 : 2;     // (gaussian: every sample is in every list)
    int by_grid = 4;
    while (by_grid > 1 && (int64_t)cb->v.ngroups * (cb->v.d / (128 * by_grid)) < 1024) by_grid >>= 1;
    p.ntw = std::min(p.ntw, std::min(by_len, by_grid));
    p.grid = dim3((unsigned)(cb->v.ngroups * (cb->v.d / (128 * p.ntw)))); p.block = dim3(256);
  } else if (G && !M && (cb->v.d & 3) == 0 && cb->v.d4 % 4 == 0 && count <= ds->n && ds->n < (1ll << 31) && !getenv("SOMHIP_UPD_LDS")) {
    // gaussian, no masks: K4g, one workgroup (up to 16 waves) per row group so that the rates are computed once; K4h:
    // the run in one piece in the data set and smaller than 4 GiB, 32 dims per wave
    const int64_t f0 = data_first % ds->n;
    p.apply = cb->v.d4 % 8 == 0 && f0 + count <= ds->n && count * (int64_t)cb->v.d * 4 < (1ll << 32) ? APPLY_GAUSS_H : APPLY_GAUSS_S;
    const int gq = p.apply == APPLY_GAUSS_H ? 8 : 4;     // chunks per wave (K4g: 8 would need 64 SGPRs for the two x buffers alone)
    const int per_row = cb->v.d4 / gq;                    // waves needed for one row group
    int nw = 1;                                           // (the most waves, up to 16, that split the row group evenly)
    for (int w = 1; w <= 16; w++) if (per_row % w == 0) nw = w;
    p.grid = dim3((unsigned)(cb->v.ngroups * (per_row / nw))); p.block = dim3(64 * nw);
  } else {
    // bubble: the scalar-operand kernel K4s when it can take the run (packed fp32: 1.44 -> 1.16 ms on the 256x256x512
    // map), else K4's LDS tiles (a shard so small that QW fell to 2: 244 vs 282 us on an eighth of the 256x256x512 map)
    p.apply = scalar_form ? APPLY_BUBBLE_S : APPLY_RUN; p.qw = QW;
    p.grid = dim3((unsigned)(cb->v.ngroups * ((cb->v.d4 + 4 * QW - 1) / (4 * QW)))); p.block = dim3(256);   // (row group, slice) items, see the kernel
  }
  return p;
}
// each stage takes its scratch slots where it starts: the lists' here, the tail starts (members) and the group order (order)
struct UpdateBufs { int2 *bxy; uint32_t *cnt; MemberEntry *lists; uint32_t *lstart, *order; };
static int bind_update(somhip_engine *e, const somhip_codebook *cb, int64_t count, UpdateBufs *b) {
  *b = UpdateBufs{};
  CHK(scratch(e, SLOT_MEMBER_XY, (size_t)count, &b->bxy));
  CHK(scratch(e, SLOT_MEMBER_COUNT, (size_t)cb->v.ngroups, &b->cnt));
  // the lists start GEMM_FRONT_PAD entries into their region: K4m's scalar quarter loads may start before a list
  CHK(scratch(e, SLOT_MEMBER_LIST, (size_t)cb->v.ngroups * (size_t)list_stride(count) + GEMM_FRONT_PAD, &b->lists));
  b->lists += GEMM_FRONT_PAD;
  return 0;
}
static int update_members(somhip_engine *e, const somhip_codebook *cb, const somhip_dataset *ds, const UpdatePlan &p,
                          int64_t data_first, int64_t count, const uint64_t *d_keys, const StepScalars *d_sc, UpdateBufs &b,
                          int64_t lazy_trips = 0) {
  if (p.tail) CHK(scratch(e, SLOT_TAIL_START, (size_t)cb->v.ngroups, &b.lstart));
  LaunchTimer t(e, KID_MEMBERS);
  return with_value<1, 0>(cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN, [&](auto g) { return with_value<1024, 256>(p.members_nt, [&](auto nt) {
    return with_value<8, 4>(p.members_rr, [&](auto rr) { return with_value<1, 0>(lazy_trips > 0, [&](auto lz) {
      constexpr bool GG = decltype(g)::value != 0, LZ = decltype(lz)::value != 0; constexpr int NT = decltype(nt)::value, RR = decltype(rr)::value;
      // (8 samples per thread: bubble, 1024 threads only; lazy: bubble only -- the plan's tail mode is)
      if constexpr ((RR == 4 || (!GG && NT == 1024)) && !(GG && LZ)) {
        return LAUNCH(e, (k_som_members<GG, NT, RR, LZ>), dim3((unsigned)cb->v.ngroups), dim3(NT), 0, cb->v, count, p.decode ? b.bxy : nullptr,
                      p.decode ? nullptr : d_keys, d_sc, b.cnt, b.lists, e->d_stats, p.entry == ENTRY_SAMPLE ? (int64_t)-1 : data_first, ds->n,
                      p.entry == ENTRY_BYTE ? 4 * cb->v.d : cb->v.d >> 2, p.tail_need, b.lstart, p.gauss_gemm ? 1 : 0, p.reach_max, lazy_trips);
      } else return fail("update_members: no k_som_members<%d, %d, %d, %d> is built", (int)GG, NT, RR, (int)LZ);
  }); }); }); });
}
static int update_apply(somhip_engine *e, const somhip_codebook *cb, const somhip_dataset *ds, const UpdatePlan &p,
                        int64_t data_first, int64_t count, const StepScalars *d_sc, const UpdateBufs &b) {
  const bool G = cb->v.neigh == SOMHIP_NEIGH_GAUSSIAN, M = ds->d_mask != nullptr;
  LaunchTimer t(e, p.apply == APPLY_GEMM ? KID_SOM_UPDATE_GEMM : p.apply == APPLY_BUBBLE_S ? KID_SOM_UPDATE_BUBBLE_S : KID_SOM_UPDATE_RUN);
  // (with_value fails where the plan holds a value no launch was built for)
  if (p.apply == APPLY_GEMM)
    return with_value<4, 2, 1>(p.ntw, [&](auto n) { return with_value<1, 0>(G, [&](auto g) {
      return LAUNCH(e, (k_som_update_gemm<decltype(n)::value, decltype(g)::value != 0>), p.grid, p.block, 0, cb->v, ds->d_rows, ds->n, data_first, count,
                    b.cnt, b.lists, b.order, e->d_stats, b.lstart);
    }); });
  if (p.apply == APPLY_GAUSS_H)
    return LAUNCH(e, k_som_update_gauss_h, p.grid, p.block, 0, cb->v, ds->d_rows + data_first % ds->n * cb->v.d, count, b.bxy, d_sc, b.cnt, b.lists,
                  b.order);
  if (p.apply == APPLY_GAUSS_S)
    return LAUNCH(e, (k_som_update_gauss_s<4>), p.grid, p.block, 0, cb->v, ds->d_rows, ds->n, data_first, count, b.bxy, d_sc, b.cnt, b.lists, b.order);
  if (p.apply == APPLY_BUBBLE_S)
    return with_value<4, 2>(p.qw, [&](auto q) { return with_value<1, 0>(p.off32, [&](auto o) {
      return LAUNCH(e, (k_som_update_bubble_s<decltype(q)::value, decltype(o)::value != 0>), p.grid, p.block, 0, cb->v, ds->d_rows, ds->n, data_first,
                    count, b.cnt, b.lists, b.order);
    }); });
  return with_value<4, 2>(p.qw, [&](auto q) { return with_value<1, 0>(G, [&](auto g) { return with_value<1, 0>(M, [&](auto m) {
    return LAUNCH(e, (k_som_update_run<decltype(q)::value, 32, decltype(g)::value != 0, decltype(m)::value != 0>), p.grid, p.block, 0, cb->v,
                  ds->d_rows, ds->d_mask, ds->n, data_first, count, b.bxy, d_sc, b.cnt, b.lists, b.order);
  }); }); });
}
// K4a over samples [from, from + n) of a run (keys, scalars and coordinates all indexed by the run's sample)
static int update_decode(somhip_engine *e, const somhip_codebook *cb, int64_t from, int64_t n, const uint64_t *d_keys,
                         const StepScalars *d_sc, const UpdateBufs &b) {
  return LAUNCH_TIMED(e, KID_DECODE, k_decode_winners, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_keys + from, d_sc + from, n, cb->v.xdim,
                      b.bxy + from);
}
// K4c (fold_held: a lazy members pass is kept, what it counted goes into the statistics) and the apply kernel
static int update_order_apply(somhip_engine *e, const somhip_codebook *cb, const somhip_dataset *ds, const UpdatePlan &p,
                              int64_t data_first, int64_t count, const StepScalars *d_sc, UpdateBufs &b, bool fold_held) {
  if (p.order) {
    CHK(scratch(e, SLOT_STAGE, (size_t)cb->v.ngroups, &b.order));
    LaunchTimer t(e, KID_DECODE);                          // (timed with k_decode_winners)
    const dim3 grid((unsigned)((cb->v.ngroups * 8 + 255) / 256));
    if (fold_held) CHK(LAUNCH(e, k_order_groups<true>, grid, dim3(256), 0, b.cnt, (int)cb->v.ngroups, b.order, e->d_stats));
    else CHK(LAUNCH(e, k_order_groups<false>, grid, dim3(256), 0, b.cnt, (int)cb->v.ngroups, b.order, nullptr));
  } else if (fold_held) {
    CHK(LAUNCH(e, k_fold_update_stats, dim3(1), dim3(256), 0, e->d_stats));
  }
  return update_apply(e, cb, ds, p, data_first, count, d_sc, b);
}
static int som_update_planned(somhip_codebook *cb, somhip_dataset *ds, const UpdatePlan &p, int64_t data_first, int64_t count,
                              const uint64_t *d_keys, const StepScalars *d_sc) {
  somhip_engine *e = cb->e;
  rows_written(cb);
  UpdateBufs b; CHK(bind_update(e, cb, count, &b));
  if (p.decode) CHK(update_decode(e, cb, 0, count, d_keys, d_sc, b));
  CHK(update_members(e, cb, ds, p, data_first, count, d_keys, d_sc, b));
  return update_order_apply(e, cb, ds, p, data_first, count, d_sc, b, false);
}
static int som_update_run(somhip_codebook *cb, somhip_dataset *ds, int64_t data_first, int64_t count,
                          const uint64_t *d_keys, const StepScalars *d_sc, const StepScalars *h_sc) {
  return som_update_planned(cb, ds, som_update_plan(cb, ds, data_first, count, h_sc), data_first, count, d_keys, d_sc);
}

// ---------------------------------------------------------------------------------
// Lazy search (som_train_batched): winners only for the end of a run.
//
// With the GEMM update in tail mode nothing reads the winner of a sample that lies in front of every row group's list
// tail: K4b walks the run from its end in trips and a group stops after the trip in which its tail holds tail_need
// entries with every live unit; K4m starts at the list's end and stops inside that tail.  So the run's last M samples
// are searched, M whole trips, and K4b runs over exactly those trips (k_som_members, lazy_trips) -- with the whole run's
// plan, count, scalars and data offsets, the keys and the decoded coordinates at the run's own indices.  A group that
// has `enough` after trip k <= M / trip has seen the same samples in the same trips as with every winner known: the same
// entries at the same places, the same count and the same lstart, and K4m's walk over them is the same walk -- the
// codebook the run leaves is the same, bit for bit, and so are the lists the statistics describe.  K4b counts the groups
// that left WITHOUT `enough`; the host reads that one word (the only host wait of the training loop, and only in lazy
// runs).  Zero: on to K4c and K4m.  Otherwise the other count - M samples are searched against the same codebook (the
// prepared copies are still valid: nothing has written it) and decode and K4b run again over the whole run, as in a
// run that was never lazy; what the first pass had counted is dropped.  A group that no winner comes near never has
// `enough`: a map whose winners all keep away from some patch -- data in one corner of a map wider than the radius,
// clustered data early in a schedule -- takes that second path in every lazy run, and pays one members pass and one
// host wait per run (about 0.15 ms at the benchmark's shape) for nothing.
//
// M: a corner patch decides -- it sees a quarter of the disc of winners that cover it whole.  With the winners spread
// evenly, the share of samples that fill a corner patch is a quarter of the plan's own `full` (area(radius - 6) /
// units), so tail_need of them are expected within tail_need / (full / 4) samples; times LAZY_MARGIN; then whole trips.
// Lazy only if that is at most half the run.  Winners are not spread evenly -- every group has to fill, and the slowest
// one needs several times what the average one does -- hence the margin.  It is TUNED ON ONE DATA SET: the benchmark's
// 10 M-vector schedule on the 65536 x 512 map, partly from a table computed from measured per-batch needs
// (profiles/lazy_search_vs_parent.txt has the measurements and the other margins).  On maps of 512 row groups and
// more, trips of 1024 x 8 are never lazy with it (the plan takes them where tail_need > 3 x 1024 x full, and M would be
// above the longest run the GEMM update takes); maps below 512 row groups take such trips from 16384 samples on
// whatever the radius, and are lazy there with M = 8192.
// ---------------------------------------------------------------------------------
constexpr double LAZY_MARGIN = 7.0;
static int64_t som_lazy_samples(const somhip_codebook *cb, const UpdatePlan &p, int64_t count, const StepScalars *h_sc) {
  if (p.apply != APPLY_GEMM || !p.tail || p.tail_need == 0) return 0;
  const int64_t trip = (int64_t)p.members_nt * p.members_rr;
  const double r = std::sqrt((double)std::max(h_sc[count - 1].thresh, 0.0f)) - 6.0;     // (the run's smallest radius)
  if (!(r > 0.0)) return 0;
  const double quarter = std::min(1.0, 0.25 * 3.6276 * r * r / std::max<double>(1.0, (double)cb->v.xdim * cb->ydim));
  const double want = LAZY_MARGIN * (double)p.tail_need / quarter;
  if (!(want <= (double)count)) return 0;
  const int64_t m = ((int64_t)std::ceil(want) + trip - 1) / trip * trip;
  return 2 * m <= count ? m : 0;
}
// one lazy run: d_keys has room for the run's keys + 4 in front and, behind `spare`, for the run's keys again
static int som_lazy_run(somhip_codebook *cb, somhip_dataset *ds, const UpdatePlan &p, int64_t row0, int64_t count, int64_t m,
                        uint64_t *d_keys, uint64_t *spare, const StepScalars *d_sc) {
  somhip_engine *e = cb->e;
  // the run's key array starts so that its searched end is aligned like the buffer itself (4 keys = 32 bytes: m is whole 1024s)
  uint64_t *kv = d_keys + ((4 - count % 4) & 3);
  const int64_t head = count - m;
  if (!e->lazy_hflag) HIPCHK(hipHostMalloc((void **)&e->lazy_hflag, sizeof(unsigned long long), hipHostMallocDefault));
  // (the held counts and the short-tail word start at zero whatever an earlier call left: an error between a members pass and its fold)
  HIPCHK(hipMemsetAsync(e->d_stats + STAT_UPDATE_HELD, 0, sizeof(unsigned long long) * (2 * STAT_UPDATE_PAIRS + 1), e->stream));
  CHK(scan_keys_top1(cb, ds, (row0 + head) % ds->n, m, kv + head));
  UpdateBufs b; CHK(bind_update(e, cb, count, &b));
  if (p.decode) CHK(update_decode(e, cb, head, m, kv, d_sc, b));
  CHK(update_members(e, cb, ds, p, row0, count, kv, d_sc, b, m / ((int64_t)p.members_nt * p.members_rr)));
  CHK(to_host_sync(e, e->lazy_hflag, e->d_stats + STAT_LAZY_SHORT, 1));
  const bool redo = *e->lazy_hflag != 0;
  if (redo) {
    // (into the spare keys, then copied: the head of the run's key array is not aligned like the buffer)
    HIPCHK(hipMemsetAsync(e->d_stats + STAT_UPDATE_HELD, 0, sizeof(unsigned long long) * (2 * STAT_UPDATE_PAIRS + 1), e->stream));
    CHK(scan_keys_top1(cb, ds, row0, head, spare));
    CHK(on_device(e, kv, spare, (size_t)head));
    if (p.decode) CHK(update_decode(e, cb, 0, head, kv, d_sc, b));
    CHK(update_members(e, cb, ds, p, row0, count, kv, d_sc, b));
  }
  rows_written(cb);
  return update_order_apply(e, cb, ds, p, row0, count, d_sc, b, !redo);
}
// the plan som_update_run makes for a run (somhip.h): the same checks as somhip_som_batch_update, host arithmetic only
extern "C" int somhip_debug_update_plan(somhip_codebook *cb, somhip_dataset *ds, const somhip_som_params *p, int64_t batch_start_iter,
                                        int64_t count, int64_t data_first, int32_t *out) try {
  CHK(check_pair(cb, ds, "somhip_debug_update_plan"));
  if (cb->v.topol < SOMHIP_TOPOL_HEXA) return fail("somhip_debug_update_plan: codebook is not a map");
  if (!p || !out || count <= 0) return fail("somhip_debug_update_plan: null argument, or count %lld < 1", (long long)count);
  std::vector<StepScalars> sc((size_t)count);
  CHK(som_scalars(lattice_of(cb), ds, p, batch_start_iter, count, data_first % ds->n, sc.data()));
  const UpdatePlan u = som_update_plan(cb, ds, data_first % ds->n, count, sc.data());
  const int32_t v[16] = {u.apply, u.qw, u.off32, u.ntw, u.decode, u.members_nt, u.members_rr, u.entry, u.gauss_gemm, u.tail,
                         (int32_t)u.tail_need, u.reach_max, u.order, (int32_t)u.grid.x, (int32_t)u.block.x, 0};
  memcpy(out, v, sizeof v);
  return 0;
} ABI_CATCH(somhip_debug_update_plan)

extern "C" int somhip_som_batch_update(somhip_codebook *cb, somhip_dataset *ds,
                                       const somhip_som_params *p, int64_t batch_start_iter,
                                       int64_t count, int64_t data_first, const uint64_t *dev_keys) try {
  CHK(check_pair(cb, ds, "somhip_som_batch_update"));
  if (cb->v.topol < SOMHIP_TOPOL_HEXA) return fail("somhip_som_batch_update: codebook is not a map");
  if (count <= 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  StepScalars *dsc; void *hsc;
  int slot;
  CHK(scratch(e, SLOT_CALL_B, (size_t)count, &dsc));
  CHK(pin_acquire(e, sizeof(StepScalars) * (size_t)count, &hsc, &slot));
  CHK(som_scalars(lattice_of(cb), ds, p, batch_start_iter, count, data_first % ds->n, (StepScalars *)hsc));
  CHK(pin_upload(e, slot, dsc, (size_t)count));
  return som_update_run(cb, ds, data_first % ds->n, count, dev_keys, (const StepScalars *)dsc, (const StepScalars *)hsc);   // asynchronous
} ABI_CATCH(somhip_som_batch_update)

// ---------------------------------------------------------------------------------
// SOMHIP_BATCH_AUTO (somhip.h): the engine's own mini-batch schedule -- a RULE in (units N, radius(t), alpha(t)), round 3.
//
// The reference is strictly online (som_rout.c:600-662); winners found against a codebook that is a batch old are a
// perturbation of it.  What a perturbation made at iteration t does to the final map is governed by
//   h(t)  = share of the map one sample teaches = min(1, area(radius(t)) / N), area = the units within the radius
//           (hexa 1 + 2 pi / sqrt 3 r^2, rect 1 + pi r^2; gaussian: the sum of its weights, twice that);
//   F(t)  = sum over t' >= t of alpha(t') h(t'): every later hit of a unit pulls it (1 - alpha) of the way off its old
//           position, so what iteration t left in a unit is scaled by exp(-F(t)) by the end of the run.
// LONG batches (32768) run while F(t) >= AUTO_FORGET = 64, SHORT ones (a quarter of that) after.  Where the line lies was
// MEASURED, at configs[3]'s real length on three (stream, init) seed pairs against the online engine
// (profiles/r03_conformity_*.jsonl, r03_switch_point_sweep.txt): the final qerror of ANY batch > 1 -- batch 256 with the
// exact update kernels included -- differs from the online one by a chaotic +-4e-4 (per-sample distances decorrelate, rms
// 0.042; two schedules whose switch point differs by one batch differ by up to 3e-4); with the long batches ending at
// 60 ... 87.5 % of the run (F = 1400 ... 35) the mean over the seeds is inside +-1e-4 of zero, at 90 % (F = 15) it is
// +1.4e-4, at 90.1 % (F = 13) +3.4e-4, at 93 % (F = 2.7) +2.4e-3: a positive bias sets in below F ~ 15.  F = 64 keeps a
// factor e^50 between the rule and that onset; short batches of 8192 or 4096 behind it: no difference beyond the noise.
// The rule is vouched for where it was measured: maps of >= 16384 units whose long phase holds >= 64 long batches.
// Everywhere else -- configs[1] (1024 units, 100 000 vectors: the qerror of every batch > 1 tried differs from the online
// one by more than 1e-4, profiles/r01_batch_study_32x32x128.txt) -- `auto` means batch 1: the reference's own schedule
// on the online engine.
// ---------------------------------------------------------------------------------
constexpr int64_t AUTO_B_LONG = 32768;
constexpr double AUTO_FORGET = 64.0;
constexpr int64_t AUTO_TAIL_DIV = 4;
constexpr int64_t AUTO_MIN_UNITS = 16384, AUTO_MIN_LONG_BATCHES = 64;
struct AutoPlan { int64_t t1 = 0, b_long = 1, b_tail = 1; bool online = true; };
static double auto_alpha(const somhip_som_params *p, double t) {
  const double L = (double)p->length;
  if (p->alpha_type == SOMHIP_ALPHA_INVERSE_T) { const double c = L / 100.0; return (double)p->alpha * c / (c + t); }   // lvq_pak.c:914-921
  return (double)p->alpha * (L - t) / L;                                                                                  // lvq_pak.c:903-906
}
static double auto_share(const somhip_som_params *p, double t, int64_t n_units, int topol, int neigh) {
  const double L = (double)p->length;
  const double r = 1.0 + ((double)p->radius - 1.0) * (L - t) / L;                                                          // som_rout.c:615
  double area = 1.0 + (topol == SOMHIP_TOPOL_RECT ? 3.14159265358979 : 3.62759872846844) * r * r;
  if (neigh == SOMHIP_NEIGH_GAUSSIAN) area *= 2.0;
  return std::min(1.0, area / (double)std::max<int64_t>(n_units, 1));
}
static AutoPlan som_auto_plan(const somhip_som_params *p, int64_t n_units, int topol, int neigh) {
  AutoPlan pl;
  const int64_t L = p->length;
  if (n_units < AUTO_MIN_UNITS || L < AUTO_MIN_LONG_BATCHES * AUTO_B_LONG || !(p->alpha > 0.0f) || !(p->radius >= 1.0f)) return pl;
  // F over the batch boundaries of the long phase, from the end of the run backwards (midpoint rule per long batch)
  const int64_t nb = L / AUTO_B_LONG;
  double F = 0.0;
  {
    const double tail0 = (double)(nb * AUTO_B_LONG), mid = 0.5 * (tail0 + (double)L);
    F += auto_alpha(p, mid) * auto_share(p, mid, n_units, topol, neigh) * ((double)L - tail0);
  }
  int64_t k = nb;                                          // the long phase is [0, k * B_LONG)
  while (k > 0 && F < AUTO_FORGET) {
    const double mid = ((double)k - 0.5) * (double)AUTO_B_LONG;
    F += auto_alpha(p, mid) * auto_share(p, mid, n_units, topol, neigh) * (double)AUTO_B_LONG;
    k--;
  }
  if (k < AUTO_MIN_LONG_BATCHES) return pl;                // too little of the run can take long batches: nothing vouched for
  pl.t1 = k * AUTO_B_LONG;
  pl.b_long = AUTO_B_LONG;
  pl.b_tail = AUTO_B_LONG / AUTO_TAIL_DIV;
  pl.online = false;
  return pl;
}
static void som_auto_batch(const AutoPlan &pl, int64_t length, int64_t it, int64_t *start, int64_t *len) {
  int64_t s, b;
  if (pl.online) { s = it; b = 1; }
  else if (it < pl.t1) { b = pl.b_long; s = it - it % b; }
  else { b = pl.b_tail; s = pl.t1 + (it - pl.t1) / b * b; }
  *start = s;
  *len = std::min(b, length - s);
}
extern "C" int somhip_som_auto_batch(const somhip_som_params *p, int64_t n_units, int topol, int neigh, int64_t iter,
                                     int64_t *batch_start, int64_t *batch_len) try {
  if (!p || p->length <= 0 || iter < 0 || iter >= p->length || n_units <= 0 || !batch_start || !batch_len)
    return fail("somhip_som_auto_batch: bad argument");
  som_auto_batch(som_auto_plan(p, n_units, topol, neigh), p->length, iter, batch_start, batch_len);
  return 0;
} ABI_CATCH(somhip_som_auto_batch)

static int som_train_batched(somhip_codebook *cb, somhip_dataset *ds, const somhip_som_params *p,
                             int32_t *trace_index, float *trace_diff) {
  somhip_engine *e = cb->e;
  const bool auto_b = p->batch == SOMHIP_BATCH_AUTO;
  const AutoPlan plan = auto_b ? som_auto_plan(p, cb->n_global, cb->v.topol, cb->v.neigh) : AutoPlan();
  const int64_t B = auto_b ? AUTO_B_LONG : p->batch;        // the longest batch of the run
  uint64_t *dkeys; StepScalars *dsc;
  const size_t kspare = ((size_t)B + 4 + 31) & ~(size_t)31;   // (lazy runs: som_lazy_run)
  CHK(scratch(e, SLOT_CALL_A, kspare + (size_t)B, &dkeys));
  CHK(scratch(e, SLOT_CALL_B, (size_t)B, &dsc));
  std::vector<uint64_t> hk((size_t)B);
  const bool trace = trace_index || trace_diff;
  // batches are aligned to the schedule (iteration 0, B, 2B, ...), as in the oracle; the host runs
  // ahead of the GPU (scalars go through a ring of pinned buffers) unless a trace is wanted
  for (int64_t off = 0; off < p->count;) {
    int64_t it0 = p->start_iter + off;
    int64_t bstart = it0 - it0 % B, blen = B;
    if (auto_b) som_auto_batch(plan, p->length, it0, &bstart, &blen);
    int64_t c = std::min(bstart + blen - it0, p->count - off);
    int64_t row0 = (p->data_first + off) % ds->n;
    void *hscv;
    int slot;
    CHK(pin_acquire(e, sizeof(StepScalars) * (size_t)c, &hscv, &slot));
    StepScalars *hsc = (StepScalars *)hscv;
    CHK(som_scalars(lattice_of(cb), ds, p, it0, c, row0, hsc));
    CHK(pin_upload(e, slot, dsc, (size_t)c));
    const UpdatePlan up = som_update_plan(cb, ds, row0, c, hsc);
    // no trace wanted and the update reads only the end of the run: only that end is searched (som_lazy_run)
    const int64_t lazy_m = trace ? 0 : som_lazy_samples(cb, up, c, hsc);
    if (lazy_m > 0) CHK(som_lazy_run(cb, ds, up, row0, c, lazy_m, dkeys, dkeys + kspare, (const StepScalars *)dsc));
    else {
      CHK(scan_keys_top1(cb, ds, row0, c, dkeys));
      CHK(som_update_planned(cb, ds, up, row0, c, (const uint64_t *)dkeys, (const StepScalars *)dsc));
    }
    if (trace) {
      CHK(to_host_sync(e, hk.data(), dkeys, (size_t)c));
      som_trace(hsc, hk.data(), c, off, trace_index, trace_diff);
    }
    off += c;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

extern "C" int somhip_som_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_som_params *p,
                                int32_t *trace_index, float *trace_diff) try {
  CHK(check_pair(cb, ds, "somhip_som_train"));
  if (!p) return fail("somhip_som_train: null params");
  if (cb->v.topol < SOMHIP_TOPOL_HEXA || (cb->v.neigh != SOMHIP_NEIGH_BUBBLE && cb->v.neigh != SOMHIP_NEIGH_GAUSSIAN))
    return fail("som_training: can't set SOM parameters");                 // som_rout.c:576-580
  if (p->length <= 0 || p->count < 0 || p->start_iter < 0 || p->start_iter + p->count > p->length)
    return fail("somhip_som_train: iterations [%lld,%lld) outside schedule of %lld",
                (long long)p->start_iter, (long long)(p->start_iter + p->count), (long long)p->length);
  if (is_shard(cb))
    return fail("somhip_som_train: sharded codebook -- use somhip_batch_winner_keys + somhip_som_batch_update");
  if (p->count == 0) return 0;
  HIPCHK(hipSetDevice(cb->e->device));
  // batch 1, or SOMHIP_BATCH_AUTO where the rule does not vouch for mini-batches: the reference's own schedule
  const bool online = p->batch == SOMHIP_BATCH_AUTO ? som_auto_plan(p, cb->n_global, cb->v.topol, cb->v.neigh).online : p->batch <= 1;
  return online ? som_train_online(cb, ds, p, trace_index, trace_diff) : som_train_batched(cb, ds, p, trace_index, trace_diff);
} ABI_CATCH(somhip_som_train)
