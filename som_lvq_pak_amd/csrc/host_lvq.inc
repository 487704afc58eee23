// host_lvq.inc -- lvq*_training: exact batched engine and the one-launch-per-iteration engine
// (included by somhip.hip: one translation unit, shared static helpers)

// ---------------------------------------------------------------------------------
// lvq*_training
// ---------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------
// lvq1/olvq1/lvq2/lvq3_training, exact batched form (kernels.hpp K6): per batch one
// frozen-codebook top-8 scan, then k_lvq_batch_apply walks the samples in order.  The
// device tells how many samples it could certify (ctl.consumed); the next batch starts
// there.  Bit-identical to the online loop.
// ---------------------------------------------------------------------------------
static int lvq_cache_slots(int d4) {
  const int64_t budget = LVQ_DYN_LDS;                // dynamic LDS; ~8.5 KiB static on top (160 KiB per workgroup)
  int64_t s = (budget - 3 * (int64_t)d4 * 16) / ((int64_t)d4 * 16);
  return (int)std::min<int64_t>(s, LVQ_BT);
}

// device buffers of one batch of the exact LVQ engine
struct LvqBatchBufs {
  float *rho, *xnorm; uint32_t *adj; int32_t *comp_samples; LvqBatchOut *out;
  float4 *stage_rows; int32_t *stage_rowid; float *stage_ta;
  int32_t *cand_lab; float *cand_ta; int32_t *mod_rows, *mod_count; float *amax_dev;
};
static int lvq_batch_bufs(somhip_engine *e, int d4, LvqBatchBufs *b) {
  void *p;
  CHK(engine_scratch(e, SLOT_LVQ_RHO, sizeof(float) * 2 * LVQ_BMAX + 16, &p)); b->rho = (float *)p; b->xnorm = b->rho + LVQ_BMAX; b->amax_dev = b->xnorm + LVQ_BMAX;
  CHK(engine_scratch(e, SLOT_LVQ_ADJ, sizeof(uint32_t) * LVQ_BMAX * LVQ_AW, &p)); b->adj = (uint32_t *)p;
  CHK(engine_scratch(e, SLOT_LVQ_COMP, sizeof(int32_t) * LVQ_BMAX, &p)); b->comp_samples = (int32_t *)p;
  CHK(engine_scratch(e, SLOT_LVQ_OUT, sizeof(LvqBatchOut), &p)); b->out = (LvqBatchOut *)p;
  CHK(engine_scratch(e, SLOT_LVQ_STAGE_ROWS, sizeof(float4) * 2 * LVQ_BMAX * (size_t)d4, &p)); b->stage_rows = (float4 *)p;
  CHK(engine_scratch(e, SLOT_LVQ_STAGE_ROWID, sizeof(int32_t) * 2 * LVQ_BMAX, &p)); b->stage_rowid = (int32_t *)p;
  CHK(engine_scratch(e, SLOT_LVQ_STAGE_TA, sizeof(float) * 2 * LVQ_BMAX, &p)); b->stage_ta = (float *)p;
  CHK(engine_scratch(e, SLOT_LVQ_CAND_LAB, sizeof(int32_t) * LVQ_BMAX * LVQ_K0, &p)); b->cand_lab = (int32_t *)p;
  CHK(engine_scratch(e, SLOT_LVQ_CAND_TA, sizeof(float) * LVQ_BMAX * LVQ_K0, &p)); b->cand_ta = (float *)p;
  CHK(engine_scratch(e, SLOT_LVQ_MOD, sizeof(int32_t) * (2 * LVQ_BMAX + 4), &p)); b->mod_rows = (int32_t *)p; b->mod_count = b->mod_rows + 2 * LVQ_BMAX;
  return 0;
}

// relation (*) over all pairs of the batch: Gram form on the matrix pipe where the shape allows (SOMHIP_LVQ_PAIRS_VALU=1:
// always the direct-form kernel); masked data: the direct-form kernel over the components both samples have
static int lvq_launch_pair_adj(somhip_engine *e, somhip_dataset *ds, const LvqBatchBufs &b, int64_t row0, int c) {
  const unsigned nt = (unsigned)((c + 63) / 64);
  if (ds->d_mask)
    hipLaunchKernelGGL(k_lvq_pair_adj<true>, dim3(nt, nt), dim3(256), 0, e->stream, ds->d_rows, ds->n, ds->d, row0, c,
                       (const float *)b.rho, b.adj, (const uint8_t *)ds->d_mask);
  else if (ds->d % 8 == 0 && !getenv("SOMHIP_LVQ_PAIRS_VALU"))
    hipLaunchKernelGGL(k_lvq_pair_adj_mfma, dim3(nt, nt), dim3(256), 0, e->stream, ds->d_rows, ds->n, ds->d, row0, c,
                       (const float *)b.rho, (const float *)b.xnorm, b.adj);
  else
    hipLaunchKernelGGL(k_lvq_pair_adj<false>, dim3(nt, nt), dim3(256), 0, e->stream, ds->d_rows, ds->n, ds->d, row0, c,
                       (const float *)b.rho, b.adj);
  HIPCHK(hipGetLastError());
  return 0;
}

// the walk's row cache and the component kernel's adjacency rows need more dynamic LDS than the default limit
static int lvq_set_attrs(somhip_engine *e) {
  if (e->lvq_apply_attr_set) return 0;                    // per engine (= per device), not per process
  HIPCHK(hipFuncSetAttribute((const void *)k_lvq_batch_apply<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LVQ_DYN_LDS));
  HIPCHK(hipFuncSetAttribute((const void *)k_lvq_batch_apply<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LVQ_DYN_LDS));
  HIPCHK(hipFuncSetAttribute((const void *)k_lvq_components, hipFuncAttributeMaxDynamicSharedMemorySize, LVQ_BMAX * LVQ_AW * 4));
  e->lvq_apply_attr_set = true;
  return 0;
}

// rho_j of relation (*) for every sample of the batch (masked data: the sample's norm over its own components)
static int lvq_launch_sample_rho(somhip_engine *e, somhip_dataset *ds, const LvqBatchBufs &b, int64_t row0, int c,
                                 const uint64_t *d_cand, float amax, bool amax_on_device) {
  const float *amax_dev = amax_on_device ? (const float *)b.amax_dev : (const float *)nullptr;
  if (ds->d_mask)
    hipLaunchKernelGGL(k_lvq_sample_rho<true>, dim3((unsigned)((c + 3) / 4)), dim3(256), 0, e->stream, ds->d_rows, ds->n, ds->d,
                       row0, c, d_cand, amax, amax_dev, b.rho, b.xnorm, (const uint8_t *)ds->d_mask);
  else
    hipLaunchKernelGGL(k_lvq_sample_rho<false>, dim3((unsigned)((c + 3) / 4)), dim3(256), 0, e->stream, ds->d_rows, ds->n, ds->d,
                       row0, c, d_cand, amax, amax_dev, b.rho, b.xnorm);
  HIPCHK(hipGetLastError());
  return 0;
}

// the walk itself: one workgroup per component (k_lvq_batch_apply<true> stages the sample's mask row beside the sample)
static int lvq_launch_walk(somhip_codebook *cb, somhip_dataset *ds, const LvqBatchBufs &b, const LvqStep *d_st, int64_t row0,
                           int c, int limit, int knn, const uint64_t *d_cand, const int32_t *d_lab, const float *d_ta,
                           const float4 *d_xrows, int xc, uint64_t *d_fin) {
  somhip_engine *e = cb->e;
  const int slots = lvq_cache_slots(cb->v.d4);
  const size_t dyn = ((size_t)cb->v.d4 * slots + 3 * (size_t)cb->v.d4) * sizeof(float4);
  LaunchTimer t(e, KID_LVQ_BATCH_APPLY);
  if (ds->d_mask)
    hipLaunchKernelGGL(k_lvq_batch_apply<true>, dim3((unsigned)c), dim3(LVQ_BT), dyn, e->stream, cb->v, ds->d_rows, ds->n, row0,
                       limit, d_lab, d_ta, d_xrows, xc, d_cand, d_st, knn, slots, (const int32_t *)b.comp_samples, d_fin,
                       b.stage_rows, b.stage_rowid, b.stage_ta, b.out, (const uint8_t *)ds->d_mask);
  else
    hipLaunchKernelGGL(k_lvq_batch_apply<false>, dim3((unsigned)c), dim3(LVQ_BT), dyn, e->stream, cb->v, ds->d_rows, ds->n, row0,
                       limit, d_lab, d_ta, d_xrows, xc, d_cand, d_st, knn, slots, (const int32_t *)b.comp_samples, d_fin,
                       b.stage_rows, b.stage_rowid, b.stage_ta, b.out);
  HIPCHK(hipGetLastError());
  return 0;
}

// One batch of the exact engine after its candidate lists are known (kernels/lvq_batch.hpp): relation (*) ->
// components -> one workgroup per component walks its samples in order -> (repeat with the batch cut at the first
// stop, if any) -> commit the rows this shard owns.  d_cand: global top-8 keys [c][8]; d_lab / d_ta: the candidates'
// labels and OLVQ1 rates; d_xrows (sharded codebooks only): tile copies [c][xc][d4] of the xc nearest candidates.
// amax: bound on |rate| of every correction of the batch (< 0: unknown -> one component, the serial walk), or
// read from b.amax_dev when amax_on_device.  *consumed <= c samples were applied.
static int lvq_walk_batch(somhip_codebook *cb, somhip_dataset *ds, const LvqBatchBufs &b, const LvqStep *d_st, int64_t row0,
                          int c, int knn, const uint64_t *d_cand, const int32_t *d_lab, const float *d_ta,
                          const float4 *d_xrows, int xc, float amax, bool amax_on_device, uint64_t *d_fin,
                          int *consumed, int *reason, int64_t *nmod_bound) {
  somhip_engine *e = cb->e;
  CHK(lvq_set_attrs(e));
  const bool single = getenv("SOMHIP_LVQ_SERIAL") != nullptr;
  {
    LaunchTimer t(e, KID_LVQ_COMPONENTS);
    if (!single) {
      CHK(lvq_launch_sample_rho(e, ds, b, row0, c, d_cand, amax, amax_on_device));
      CHK(lvq_launch_pair_adj(e, ds, b, row0, c));
    }
    hipLaunchKernelGGL(k_lvq_components, dim3(1), dim3(LVQ_BMAX), (size_t)c * LVQ_AW * 4, e->stream, (const uint32_t *)b.adj, c,
                       single ? 1 : 0, b.comp_samples, b.out);
  }
  HIPCHK(hipGetLastError());
  static_assert(sizeof(LvqBatchOut) < 32768, "summary block");
  std::vector<char> hbuf(sizeof(LvqBatchOut));
  LvqBatchOut *ho = reinterpret_cast<LvqBatchOut *>(hbuf.data());
  int limit = c;
  for (int pass = 0; pass < 2; pass++) {
    CHK(lvq_launch_walk(cb, ds, b, d_st, row0, c, limit, knn, d_cand, d_lab, d_ta, d_xrows, xc, d_fin));
    HIPCHK(hipMemcpyAsync(ho, b.out, sizeof(LvqBatchOut), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (ho->ncomp < 1 || ho->ncomp > c) return fail("somhip_lvq_train: bad component count %d", ho->ncomp);
    int first_stop = 0x7FFFFFFF, why = 0;
    for (int k = 0; k < ho->ncomp; k++)
      if (ho->stop[k] < first_stop) { first_stop = ho->stop[k]; why = ho->reason[k]; }
    if (first_stop >= limit) break;                       // every component walked to the end (of the cut batch)
    if (pass == 1) return fail("somhip_lvq_train: a component stopped again after the batch was cut (sample %d)", first_stop);
    *reason = why;
    limit = first_stop;                                   // the walk is deterministic: samples < limit come out the same
    if (limit == 0) break;                                // nothing can be applied (cannot happen: an empty cache never blocks)
  }
  *consumed = limit;
  int64_t bound = 0;
  for (int k = 0; k < ho->ncomp; k++) bound += ho->nslots[k];
  *nmod_bound = bound;
  e->lvq_components += (uint64_t)ho->ncomp;
  int big = 0;
  for (int k = 0; k < ho->ncomp; k++) big = std::max(big, ho->start[k + 1] - ho->start[k]);
  e->lvq_largest += (uint64_t)big;
  for (int k = 0; k < 4; k++) e->lvq_cycles[k] += (uint64_t)ho->cycles[k];
  if (limit > 0 && bound > 0) {
    HIPCHK(hipMemsetAsync(b.mod_count, 0, sizeof(int32_t), e->stream));
    LaunchTimer t(e, KID_LVQ_BATCH_APPLY);
    hipLaunchKernelGGL(k_lvq_commit, dim3((unsigned)ho->ncomp), dim3(256), 0, e->stream, cb->v, (const LvqBatchOut *)b.out,
                       (const float4 *)b.stage_rows, (const int32_t *)b.stage_rowid, (const float *)b.stage_ta,
                       knn == 1 && d_ta ? cb->d_talpha : (float *)nullptr, b.mod_rows, b.mod_count);
    HIPCHK(hipGetLastError());
    // the bf16 copies / norms of exactly the rows this batch corrected, so that the next batch's pre-filter (big
    // codebooks, scan_keys_topk) needs no pass over the whole codebook -- only if they were current for the codebook
    // this batch started from (a scan that took the direct path never made them so: re-splitting a few rows of stale
    // tiles must not validate them)
    if (cb->prep_valid && cb->d_chi && cb->d_cn && e->scan_mode == SOMHIP_SCAN_MFMA_BF16) {
      hipLaunchKernelGGL(k_prep_rows_bf16, dim3((unsigned)((bound + 3) / 4)), dim3(256), 0, e->stream, cb->v,
                         (cb->v.d4 + 1) / 2, (const int32_t *)b.mod_rows, (int)bound, (const int32_t *)b.mod_count, cb->d_cn,
                         cb->d_chi, cb->d_clo);
      HIPCHK(hipGetLastError());
      cb->rowmajor_valid = false;                           // (the row-major copy is not re-split row by row)
    } else {
      cb->prep_valid = false;
    }
  }
  return 0;
}

// bound on |rate| of the batch's corrections from its step scalars (LVQ1 / LVQ2.1 / LVQ3: the schedule value, and
// alpha * epsilon); OLVQ1 rates live per row: see k_lvq_amax
static float lvq_amax_of(const LvqStep *st, int c) {
  float m = 0.0f;
  for (int j = 0; j < c; j++) {
    const float a = std::fabs(st[j].alpha), ae = std::fabs(st[j].alpha * st[j].epsilon);
    if (!(a == a) || !(ae == ae)) return -1.0f;
    m = std::max(m, std::max(a, ae));
  }
  return m;
}

// The walk of a batch as the loop below launches it when it does not wait for the host: relation (*), components,
// one walk over the whole batch, then a commit that happens only if every component ran through (k_lvq_commit with
// the control block) -- no read-back in between.  fin: where this batch's winners go (trace).
static int lvq_walk_batch_nowait(somhip_codebook *cb, somhip_dataset *ds, const LvqBatchBufs &b, const LvqStep *d_st, int64_t row0,
                                 int c, int knn, const uint64_t *d_cand, const int32_t *d_lab, const float *d_ta, float amax,
                                 bool amax_on_device, uint64_t *d_fin, LvqCtl *d_ctl, int batch_id) {
  somhip_engine *e = cb->e;
  CHK(lvq_set_attrs(e));
  {
    LaunchTimer t(e, KID_LVQ_COMPONENTS);
    CHK(lvq_launch_sample_rho(e, ds, b, row0, c, d_cand, amax, amax_on_device));
    CHK(lvq_launch_pair_adj(e, ds, b, row0, c));
    hipLaunchKernelGGL(k_lvq_components, dim3(1), dim3(LVQ_BMAX), (size_t)c * LVQ_AW * 4, e->stream, (const uint32_t *)b.adj, c,
                       0, b.comp_samples, b.out);
  }
  CHK(lvq_launch_walk(cb, ds, b, d_st, row0, c, c, knn, d_cand, d_lab, d_ta, (const float4 *)nullptr, 0, d_fin));
  HIPCHK(hipMemsetAsync(b.mod_count, 0, sizeof(int32_t), e->stream));
  {
    LaunchTimer t(e, KID_LVQ_BATCH_APPLY);
    hipLaunchKernelGGL(k_lvq_commit, dim3((unsigned)c), dim3(256), 0, e->stream, cb->v, (const LvqBatchOut *)b.out,
                       (const float4 *)b.stage_rows, (const int32_t *)b.stage_rowid, (const float *)b.stage_ta,
                       knn == 1 && d_ta ? cb->d_talpha : (float *)nullptr, b.mod_rows, b.mod_count, d_ctl, batch_id, c);
  }
  HIPCHK(hipGetLastError());
  // the bf16 copies / norms of the rows this batch corrected (see lvq_walk_batch); at most two rows per sample
  if (cb->prep_valid && cb->d_chi && cb->d_cn && e->scan_mode == SOMHIP_SCAN_MFMA_BF16) {
    hipLaunchKernelGGL(k_prep_rows_bf16, dim3((unsigned)((2 * c + 3) / 4)), dim3(256), 0, e->stream, cb->v,
                       (cb->v.d4 + 1) / 2, (const int32_t *)b.mod_rows, 2 * c, (const int32_t *)b.mod_count, cb->d_cn,
                       cb->d_chi, cb->d_clo, (const int32_t *)&d_ctl->poison);
    HIPCHK(hipGetLastError());
    cb->rowmajor_valid = false;                             // (the row-major copy is not re-split row by row)
  } else {
    cb->prep_valid = false;
  }
  return 0;
}

// The exact batched engine's loop.  Batch after batch is launched without waiting for the one before (its scalars
// go through the ring of pinned buffers, its verdict stays on the device: LvqCtl); the control block of every batch
// is read back asynchronously and looked at a few batches later.  A batch that stopped early -- rare: the candidate
// lists and the row cache are sized so that it is -- has poisoned everything launched after it; the host then redoes
// that one batch with lvq_walk_batch (which cuts it at the stop and reads the verdict back) and goes on from there.
// SOMHIP_LVQ_SYNC=1: every batch the careful way.
static int lvq_train_batched(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p, int knn,
                             float *talpha, int32_t *trace_index, float *trace_diff) {
  somhip_engine *e = cb->e;
  const int64_t BMAX = LVQ_BMAX;
  constexpr int RING = 8;
  void *dcand, *dfin, *dst, *dctl_v;
  const bool want_trace = trace_index || trace_diff;
  // no waiting only if the winners of the whole call fit a device buffer (they are read back at the end)
  const bool nowait = !getenv("SOMHIP_LVQ_SYNC") && !getenv("SOMHIP_LVQ_SERIAL") && (!want_trace || p->count <= (1ll << 22));
  CHK(engine_scratch(e, SLOT_CALL_A, sizeof(uint64_t) * (size_t)BMAX * LVQ_K0, &dcand));
  CHK(engine_scratch(e, SLOT_CALL_B, sizeof(LvqStep) * (size_t)BMAX, &dst));
  CHK(engine_scratch(e, SLOT_LVQ_FINAL, sizeof(uint64_t) * 2 * (size_t)(nowait && want_trace ? std::max<int64_t>(p->count, BMAX) : BMAX), &dfin));
  CHK(engine_scratch(e, SLOT_LVQ_CTL, sizeof(LvqCtl), &dctl_v));
  LvqCtl *dctl = (LvqCtl *)dctl_v;
  LvqBatchBufs b;
  CHK(lvq_batch_bufs(e, cb->v.d4, &b));
  if (!e->lvq_hctl) HIPCHK(hipHostMalloc((void **)&e->lvq_hctl, sizeof(LvqCtl) * RING, hipHostMallocDefault));
  for (int i = 0; i < RING; i++)
    if (!e->lvq_ev[i]) HIPCHK(hipEventCreateWithFlags(&e->lvq_ev[i], hipEventDisableTiming));
  HIPCHK(hipMemsetAsync(dctl, 0, sizeof(LvqCtl), e->stream));
  std::vector<LvqStep> hst((size_t)BMAX);
  std::vector<uint64_t> hfin;
  const float ratio = (1 - p->winlen) / (1 + p->winlen);                  // lvq_rout.c:770, fp32
  const bool olvq = p->kind == SOMHIP_OLVQ1;
  int64_t B = std::max<int64_t>(32, std::min<int64_t>(BMAX, e->lvq_batch_hint));   // what the previous call ended with
  int64_t off = 0;
  uint64_t n_sync_batches = 0;
  auto fill_steps = [&](LvqStep *st, int64_t o, int64_t c) {
    const int64_t it0 = p->start_iter + o, row0 = (p->data_first + o) % ds->n;
    for (int64_t j = 0; j < c; j++) {
      LvqStep s;
      s.kind = p->kind;
      s.alpha = alpha_at(p->alpha_type, it0 + j, p->length, p->alpha);
      s.alpha_clamp = p->alpha;
      s.win_ratio = ratio;
      s.epsilon = p->epsilon;
      s.label = ds->labels[(size_t)((row0 + j) % ds->n)];
      st[(size_t)j] = s;
    }
  };
  auto launch_front = [&](int64_t row0, int64_t c) -> int {   // candidate lists, their labels / rates, the OLVQ1 rate bound
    CHK(scan_keys_topk<LVQ_K0>(cb, ds, row0, c, (uint64_t *)dcand, knn == 2 ? 1 : 0));
    hipLaunchKernelGGL(k_lvq_cand_meta, dim3((unsigned)((c * LVQ_K0 + 255) / 256)), dim3(256), 0, e->stream, cb->v,
                       (const uint64_t *)dcand, c * LVQ_K0, knn, (const int32_t *)cb->d_labels,
                       olvq ? (const float *)cb->d_talpha : (const float *)nullptr, b.cand_lab, olvq ? b.cand_ta : (float *)nullptr);
    if (olvq)
      hipLaunchKernelGGL(k_lvq_amax, dim3(1), dim3(256), 0, e->stream, (const uint64_t *)dcand, c * LVQ_K0, (const float *)b.cand_ta,
                         p->alpha, b.amax_dev);
    HIPCHK(hipGetLastError());
    return 0;
  };
  struct Pending { int64_t off, c; int id; };
  Pending ring[RING];
  int head = 0, tail = 0, next_id = 1;                    // batches in flight: ring[tail % RING .. head % RING)
  int64_t launched = 0;                                   // samples launched so far (assuming every batch runs through)
  while (off < p->count) {
    if (nowait) {
      // ---- keep launching; look at the oldest read-back when the ring is full or nothing is left to launch
      if (launched < p->count && head - tail < RING) {
        const int64_t c = std::min(B, p->count - launched);
        const int64_t row0 = (p->data_first + launched) % ds->n;
        void *hv; int slot;
        CHK(pin_acquire(e, sizeof(LvqStep) * (size_t)c, &hv, &slot));
        fill_steps((LvqStep *)hv, launched, c);
        CHK(pin_upload(e, slot, dst, sizeof(LvqStep) * (size_t)c));
        CHK(launch_front(row0, c));
        const float amax = olvq ? 0.0f : lvq_amax_of((const LvqStep *)hv, (int)c);
        // (a rate bound < 0 -- a NaN in the schedule -- makes the whole batch one component inside k_lvq_sample_rho)
        const int id = next_id++;
        CHK(lvq_walk_batch_nowait(cb, ds, b, (const LvqStep *)dst, row0, (int)c, knn, (const uint64_t *)dcand, b.cand_lab,
                                  olvq ? b.cand_ta : (const float *)nullptr, amax, olvq,
                                  (uint64_t *)dfin + (want_trace ? 2 * launched : 0), dctl, id));
        HIPCHK(hipMemcpyAsync(&e->lvq_hctl[head % RING], dctl, sizeof(LvqCtl), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipEventRecord(e->lvq_ev[head % RING], e->stream));
        ring[head % RING] = {launched, c, id};
        head++;
        launched += c;
        B = std::min<int64_t>(BMAX, 2 * B);               // a batch that ran through doubles
        continue;
      }
      HIPCHK(hipEventSynchronize(e->lvq_ev[tail % RING]));
      const LvqCtl hc = e->lvq_hctl[tail % RING];
      const Pending pd = ring[tail % RING];
      tail++;
      if (!hc.poison) { off = pd.off + pd.c; continue; }  // confirmed
      // ---- this batch stopped early (the batches before it were confirmed clean; those after it applied nothing)
      HIPCHK(hipStreamSynchronize(e->stream));
      off = pd.off;                                       // == the poisoned batch: earlier ones were confirmed clean
      head = tail = 0;
      HIPCHK(hipMemsetAsync(dctl, 0, 4 * sizeof(int32_t), e->stream));    // clear the flag, keep the statistics
      B = pd.c;
    }
    // ---- one batch the careful way (SOMHIP_LVQ_SYNC, or the redo of a batch that stopped early)
    const int64_t c = std::min(B, p->count - off);
    const int64_t row0 = (p->data_first + off) % ds->n;
    fill_steps(hst.data(), off, c);
    HIPCHK(hipMemcpyAsync(dst, hst.data(), sizeof(LvqStep) * (size_t)c, hipMemcpyHostToDevice, e->stream));
    CHK(launch_front(row0, c));
    int consumed = 0, reason = 0;
    int64_t nmod = 0;
    uint64_t *fin_here = (uint64_t *)dfin + (nowait && want_trace ? 2 * off : 0);
    CHK(lvq_walk_batch(cb, ds, b, (const LvqStep *)dst, row0, (int)c, knn, (const uint64_t *)dcand, b.cand_lab,
                       olvq ? b.cand_ta : (const float *)nullptr, nullptr, 0, olvq ? 0.0f : lvq_amax_of(hst.data(), (int)c), olvq,
                       fin_here, &consumed, &reason, &nmod));
    if (consumed <= 0)
      // cannot happen: with an empty cache every winner comes from the frozen list and one or two slots always fit
      return fail("somhip_lvq_train: batch made no progress (reason %d)", reason);
    if (want_trace && !nowait) {
      hfin.resize((size_t)BMAX * 2);
      HIPCHK(hipMemcpy(hfin.data(), dfin, sizeof(uint64_t) * 2 * (size_t)consumed, hipMemcpyDeviceToHost));
      for (int64_t j = 0; j < consumed; j++)
        for (int k = 0; k < knn; k++) {
          int32_t idx; float df;
          decode_key(hfin[(size_t)(2 * j + k)], knn == 2, &idx, &df);
          if (trace_index) trace_index[(off + j) * knn + k] = idx;
          if (trace_diff) trace_diff[(off + j) * knn + k] = df;
        }
    }
    off += consumed;
    launched = off;
    n_sync_batches++;
    if (reason == 1) e->lvq_stop_list++;
    if (reason == 2) e->lvq_stop_cache++;
    // next batch: a little more than what this one managed (the scan of samples that were not certified is
    // wasted), never below 32; a batch that ran through doubles
    B = consumed == c ? std::min<int64_t>(BMAX, 2 * B)
                      : std::min<int64_t>(BMAX, std::max<int64_t>(32, (int64_t)consumed + consumed / 4 + 8));
  }
  // statistics of the batches that never came back to the host; the winners of the whole call
  LvqCtl fin_ctl;
  HIPCHK(hipMemcpyAsync(&fin_ctl, dctl, sizeof fin_ctl, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (fin_ctl.poison) return fail("somhip_lvq_train: a stopped batch was left behind (batch %d)", fin_ctl.batch);
  e->lvq_components += fin_ctl.comps;
  e->lvq_largest += fin_ctl.largest;
  for (int k = 0; k < 4; k++) e->lvq_cycles[k] += fin_ctl.cycles[k];
  if (nowait && want_trace) {
    hfin.resize((size_t)p->count * 2);
    HIPCHK(hipMemcpy(hfin.data(), dfin, sizeof(uint64_t) * 2 * (size_t)p->count, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < p->count; j++)
      for (int k = 0; k < knn; k++) {
        int32_t idx; float df;
        decode_key(hfin[(size_t)(2 * j + k)], knn == 2, &idx, &df);
        if (trace_index) trace_index[j * knn + k] = idx;
        if (trace_diff) trace_diff[j * knn + k] = df;
      }
  }
  e->lvq_batches += n_sync_batches + fin_ctl.batches;
  e->lvq_samples += (uint64_t)p->count;
  e->lvq_batch_hint = B;
  return 0;
}

// lvq*_training (include/somhip.h): the exact batched engine, masked data included (the sample's mask in the frozen
// scan, in relation (*) and in the walk); else -- SOMHIP_LVQ_ONLINE=1, a patch-ordered codebook, a row too long for
// the cache -- one k_lvq_online_step launch per iteration
extern "C" int somhip_lvq_train(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p,
                                float *talpha, int32_t *trace_index, float *trace_diff) try {
  CHK(check_pair(cb, ds, "somhip_lvq_train"));
  if (!p) return fail("somhip_lvq_train: null params");
  if (p->kind < SOMHIP_LVQ1 || p->kind > SOMHIP_LVQ3) return fail("Unknown LVQ type %d", p->kind);
  if (!cb->d_labels) return fail("somhip_lvq_train: codebook has no labels");
  if (ds->labels.empty()) return fail("somhip_lvq_train: data has no labels");
  if (p->kind == SOMHIP_OLVQ1 && !talpha) return fail("somhip_lvq_train: OLVQ1 needs talpha");
  if (p->length <= 0 || p->count < 0 || p->start_iter + p->count > p->length)
    return fail("somhip_lvq_train: iterations outside schedule");
  // masked data: a sample with every component masked has no winner, and the reference then adapts through a NULL
  // winner (lvq_rout.c:542-545) -- refuse such a run before anything is trained
  const bool masked = ds->d_mask != nullptr;
  if (masked && !ds->all_masked.empty())
    for (int64_t j = 0; j < std::min<int64_t>(p->count, ds->n); j++) {
      const int64_t r = (p->data_first + j) % ds->n;
      if (ds->all_masked[(size_t)r])
        return fail("somhip_lvq_train: data row %lld has every component masked: no winner (the reference crashes here)",
                    (long long)r);
    }
  if (cb->v.row_offset != 0 || cb->n_global != cb->v.n) return fail("somhip_lvq_train: sharded codebook not supported");
  const int knn = (p->kind >= SOMHIP_LVQ2) ? 2 : 1;
  if (knn == 2 && cb->v.n < 2) return fail("somhip_lvq_train: LVQ2/LVQ3 need at least two code rows");
  if (p->count == 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  if (p->kind == SOMHIP_OLVQ1) {
    if (!cb->d_talpha) HIPCHK(hipMalloc((void **)&cb->d_talpha, sizeof(float) * (size_t)cb->v.n));
    HIPCHK(hipMemcpyAsync(cb->d_talpha, talpha, sizeof(float) * (size_t)cb->v.n, hipMemcpyHostToDevice, e->stream));
  }
  // exact batched engine unless asked otherwise (SOMHIP_LVQ_ONLINE=1) or the row does not fit the cache
  if (!getenv("SOMHIP_LVQ_ONLINE") && cb->v.patch_w == 0 && cb->v.d4 <= LVQ_BT && lvq_cache_slots(cb->v.d4) >= 8) {
    int rc = lvq_train_batched(cb, ds, p, knn, talpha, trace_index, trace_diff);
    if (rc) return rc;
    if (p->kind == SOMHIP_OLVQ1)
      HIPCHK(hipMemcpyAsync(talpha, cb->d_talpha, sizeof(float) * (size_t)cb->v.n, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return 0;
  }
  cb->prep_valid = false;                                 // the per-iteration kernel rewrites rows in place
  auto step = masked ? k_lvq_online_step<true> : k_lvq_online_step<false>;
  const int64_t CH = 4096;
  const int nblk = (int)((cb->v.ngroups + 3) / 4);
  void *dpart, *dfinal, *dst;
  CHK(engine_scratch(e, SLOT_PARTIAL, sizeof(uint64_t) * (size_t)nblk * 2 * 2, &dpart));
  CHK(engine_scratch(e, SLOT_CALL_A, sizeof(uint64_t) * (size_t)(CH + 1) * 2, &dfinal));
  CHK(engine_scratch(e, SLOT_CALL_B, sizeof(LvqStep) * (size_t)(CH + 1), &dst));
  uint64_t *part[2] = {(uint64_t *)dpart, (uint64_t *)dpart + (size_t)nblk * 2};
  uint64_t *fin = (uint64_t *)dfinal;
  LvqStep *st = (LvqStep *)dst;
  std::vector<LvqStep> hst((size_t)CH + 1);
  std::vector<uint64_t> hfin((size_t)(CH + 1) * 2);
  const float ratio = (1 - p->winlen) / (1 + p->winlen);                  // lvq_rout.c:770, fp32
  int64_t prev_row = 0;
  bool have_prev = false;
  int flip = 0;
  // fin[j] receives the merged winners of chunk-iteration j-1 when iteration j launches;
  // the last one of a chunk lands in fin[c] when the next chunk's first launch (or the
  // flush) runs, so traces are read one launch late.
  int64_t pending_trace = -1;   // global offset of the iteration whose winners arrive next
  for (int64_t off = 0; off < p->count; off += CH) {
    int64_t c = std::min(CH, p->count - off);
    int64_t it0 = p->start_iter + off, row0 = (p->data_first + off) % ds->n;
    for (int64_t j = 0; j < c; j++) {
      int64_t r = (row0 + j) % ds->n;
      LvqStep s;
      s.kind = p->kind;
      s.alpha = alpha_at(p->alpha_type, it0 + j, p->length, p->alpha);
      s.alpha_clamp = p->alpha;
      s.win_ratio = ratio;
      s.epsilon = p->epsilon;
      s.label = ds->labels[(size_t)r];
      hst[(size_t)j + 1] = s;
    }
    HIPCHK(hipMemcpyAsync(st + 1, hst.data() + 1, sizeof(LvqStep) * (size_t)c, hipMemcpyHostToDevice, e->stream));
    for (int64_t j = 0; j < c; j++) {
      int64_t cur_row = (row0 + j) % ds->n;
      {
        LaunchTimer t(e, KID_LVQ_ONLINE_STEP);
        hipLaunchKernelGGL(step, dim3((unsigned)nblk), dim3(256), 0, e->stream, cb->v,
                           ds->d_rows, (const uint8_t *)ds->d_mask, (const int32_t *)cb->d_labels, cb->d_talpha,
                           prev_row, cur_row, have_prev ? 1 : 0, 1, knn, (const uint64_t *)part[flip], nblk,
                           part[flip ^ 1], fin + 2 * j, (const LvqStep *)(st + j));
      }
      flip ^= 1;
      prev_row = cur_row;
      have_prev = true;
    }
    HIPCHK(hipGetLastError());
    // winners of iterations (off-1 .. off+c-2) are now in fin[0..c-1]
    if (trace_index || trace_diff) {
      HIPCHK(hipMemcpyAsync(hfin.data(), fin, sizeof(uint64_t) * 2 * (size_t)c, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      for (int64_t j = 0; j < c; j++) {
        int64_t it = off + j - 1;
        if (it < 0) continue;
        for (int k = 0; k < knn; k++) {
          int32_t idx; float df;
          decode_key(hfin[(size_t)(2 * j + k)], knn == 2, &idx, &df);
          if (trace_index) trace_index[it * knn + k] = idx;
          if (trace_diff) trace_diff[it * knn + k] = df;
        }
      }
    }
    HIPCHK(hipMemcpyAsync(st, st + c, sizeof(LvqStep), hipMemcpyDeviceToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    (void)pending_trace;
  }
  // flush: apply the last iteration's correction; its winners land in fin[0]
  {
    LaunchTimer t(e, KID_LVQ_ONLINE_STEP);
    hipLaunchKernelGGL(step, dim3((unsigned)nblk), dim3(256), 0, e->stream, cb->v, ds->d_rows,
                       (const uint8_t *)ds->d_mask, (const int32_t *)cb->d_labels, cb->d_talpha, prev_row, prev_row, 1,
                       0, knn, (const uint64_t *)part[flip], nblk, part[flip ^ 1], fin, (const LvqStep *)st);
  }
  HIPCHK(hipGetLastError());
  if (trace_index || trace_diff) {
    HIPCHK(hipMemcpyAsync(hfin.data(), fin, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    int64_t it = p->count - 1;
    for (int k = 0; k < knn; k++) {
      int32_t idx; float df;
      decode_key(hfin[(size_t)k], knn == 2, &idx, &df);
      if (trace_index) trace_index[it * knn + k] = idx;
      if (trace_diff) trace_diff[it * knn + k] = df;
    }
  }
  if (p->kind == SOMHIP_OLVQ1)
    HIPCHK(hipMemcpyAsync(talpha, cb->d_talpha, sizeof(float) * (size_t)cb->v.n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_lvq_train)


// ---------------------------------------------------------------------------------
// lvq*_training over a row-sharded codebook (multi-GPU): one batch in three calls, the host's
// collectives between them (include/somhip.h)
// ---------------------------------------------------------------------------------
extern "C" int somhip_lvq_rates_upload(somhip_codebook *cb, const float *talpha) try {
  if (!cb || !talpha) return fail("somhip_lvq_rates_upload: null argument");
  if (!cb->e) return fail("somhip_lvq_rates_upload: the engine of this codebook was destroyed");
  HIPCHK(hipSetDevice(cb->e->device));
  if (!cb->d_talpha) HIPCHK(hipMalloc((void **)&cb->d_talpha, sizeof(float) * (size_t)cb->v.n));
  HIPCHK(hipMemcpyAsync(cb->d_talpha, talpha, sizeof(float) * (size_t)cb->v.n, hipMemcpyHostToDevice, cb->e->stream));
  HIPCHK(hipStreamSynchronize(cb->e->stream));
  return 0;
} ABI_CATCH(somhip_lvq_rates_upload)
extern "C" int somhip_lvq_rates_download(somhip_codebook *cb, float *talpha) try {
  if (!cb || !talpha) return fail("somhip_lvq_rates_download: null argument");
  if (!cb->e) return fail("somhip_lvq_rates_download: the engine of this codebook was destroyed");
  if (!cb->d_talpha) return fail("somhip_lvq_rates_download: no rates on this codebook");
  HIPCHK(hipSetDevice(cb->e->device));
  HIPCHK(hipMemcpyAsync(talpha, cb->d_talpha, sizeof(float) * (size_t)cb->v.n, hipMemcpyDeviceToHost, cb->e->stream));
  HIPCHK(hipStreamSynchronize(cb->e->stream));
  return 0;
} ABI_CATCH(somhip_lvq_rates_download)

extern "C" int somhip_merge_topk_keys(somhip_engine *e, const uint64_t *dev_gathered, int n_shards, int64_t count, int knn,
                                      uint64_t *dev_keys) try {
  if (!e || !dev_gathered || !dev_keys) return fail("somhip_merge_topk_keys: null argument");
  if (n_shards < 1 || count < 0) return fail("somhip_merge_topk_keys: bad shape");
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(e->device));
  return with_topk_width(knn, "somhip_merge_topk_keys", [&](auto k) {
    hipLaunchKernelGGL(k_merge_shard_topk<decltype(k)::value>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, e->stream,
                       dev_gathered, n_shards, count, dev_keys);
    HIPCHK(hipGetLastError());
    return 0;
  });
} ABI_CATCH(somhip_merge_topk_keys)

extern "C" int somhip_lvq_batch_candidates(somhip_codebook *cb, int64_t count, int kind, const uint64_t *dev_keys, int xrows,
                                           int32_t *dev_lab, float *dev_ta, float *dev_rows) try {
  if (!cb || !dev_keys || !dev_lab || !dev_rows) return fail("somhip_lvq_batch_candidates: null argument");
  if (!cb->e) return fail("somhip_lvq_batch_candidates: the engine of this codebook was destroyed");
  if (kind < SOMHIP_LVQ1 || kind > SOMHIP_LVQ3) return fail("Unknown LVQ type %d", kind);
  if (count < 0 || count > LVQ_BMAX) return fail("somhip_lvq_batch_candidates: at most %d samples per batch", LVQ_BMAX);
  if (xrows < 1 || xrows > LVQ_K0) return fail("somhip_lvq_batch_candidates: xrows must be 1..%d", LVQ_K0);
  if (!cb->d_labels) return fail("somhip_lvq_batch_candidates: codebook has no labels");
  if (kind == SOMHIP_OLVQ1 && (!cb->d_talpha || !dev_ta)) return fail("somhip_lvq_batch_candidates: OLVQ1 needs rates (somhip_lvq_rates_upload)");
  if (cb->v.patch_w != 0) return fail("somhip_lvq_batch_candidates: LVQ codebooks are stored in row order");
  if (count == 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const int knn = kind >= SOMHIP_LVQ2 ? 2 : 1;
  hipLaunchKernelGGL(k_lvq_cand_meta, dim3((unsigned)((count * LVQ_K0 + 255) / 256)), dim3(256), 0, e->stream, cb->v, dev_keys,
                     count * LVQ_K0, knn, (const int32_t *)cb->d_labels, kind == SOMHIP_OLVQ1 ? (const float *)cb->d_talpha : (const float *)nullptr,
                     dev_lab, dev_ta);
  hipLaunchKernelGGL(k_lvq_cand_rows, dim3((unsigned)(count * xrows)), dim3(256), 0, e->stream, cb->v, dev_keys, (int)count, xrows, knn,
                     reinterpret_cast<float4 *>(dev_rows));
  HIPCHK(hipGetLastError());
  return 0;
} ABI_CATCH(somhip_lvq_batch_candidates)

extern "C" int somhip_lvq_batch_apply(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p,
                                      int64_t batch_start_iter, int64_t count, int64_t data_first, const uint64_t *dev_keys,
                                      const int32_t *dev_lab, const float *dev_ta, const float *dev_rows, int xrows,
                                      int64_t *consumed, int32_t *trace_index, float *trace_diff) try {
  CHK(check_pair(cb, ds, "somhip_lvq_batch_apply"));
  if (!p || !dev_keys || !dev_lab || !dev_rows || !consumed) return fail("somhip_lvq_batch_apply: null argument");
  if (p->kind < SOMHIP_LVQ1 || p->kind > SOMHIP_LVQ3) return fail("Unknown LVQ type %d", p->kind);
  if (ds->labels.empty()) return fail("somhip_lvq_batch_apply: data has no labels");
  if (count < 0 || count > LVQ_BMAX) return fail("somhip_lvq_batch_apply: at most %d samples per batch", LVQ_BMAX);
  // masked data: a sample with every component masked has no winner (see somhip_lvq_train) -- refuse the batch
  if (ds->d_mask && !ds->all_masked.empty())
    for (int64_t j = 0; j < std::min<int64_t>(count, ds->n); j++) {
      const int64_t r = (data_first + j) % ds->n;
      if (ds->all_masked[(size_t)r])
        return fail("somhip_lvq_batch_apply: data row %lld has every component masked: no winner (the reference crashes here)",
                    (long long)r);
    }
  if (xrows < 1 || xrows > LVQ_K0) return fail("somhip_lvq_batch_apply: xrows must be 1..%d", LVQ_K0);
  if (p->kind == SOMHIP_OLVQ1 && (!cb->d_talpha || !dev_ta)) return fail("somhip_lvq_batch_apply: OLVQ1 needs rates (somhip_lvq_rates_upload)");
  if (cb->v.patch_w != 0 || cb->v.d4 > LVQ_BT || lvq_cache_slots(cb->v.d4) < 8)
    return fail("somhip_lvq_batch_apply: rows of %d components do not fit the on-chip cache of the batched engine", cb->v.d);
  *consumed = 0;
  if (count == 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const int knn = p->kind >= SOMHIP_LVQ2 ? 2 : 1;
  const bool olvq = p->kind == SOMHIP_OLVQ1;
  void *dst, *dfin;
  CHK(engine_scratch(e, SLOT_CALL_B, sizeof(LvqStep) * (size_t)LVQ_BMAX, &dst));
  CHK(engine_scratch(e, SLOT_LVQ_FINAL, sizeof(uint64_t) * (size_t)LVQ_BMAX * 2, &dfin));
  LvqBatchBufs b;
  CHK(lvq_batch_bufs(e, cb->v.d4, &b));
  std::vector<LvqStep> hst((size_t)count);
  const float ratio = (1 - p->winlen) / (1 + p->winlen);                  // lvq_rout.c:770, fp32
  const int64_t row0 = data_first % ds->n;
  for (int64_t j = 0; j < count; j++) {
    LvqStep s;
    s.kind = p->kind;
    s.alpha = alpha_at(p->alpha_type, batch_start_iter + j, p->length, p->alpha);
    s.alpha_clamp = p->alpha;
    s.win_ratio = ratio;
    s.epsilon = p->epsilon;
    s.label = ds->labels[(size_t)((row0 + j) % ds->n)];
    hst[(size_t)j] = s;
  }
  HIPCHK(hipMemcpyAsync(dst, hst.data(), sizeof(LvqStep) * (size_t)count, hipMemcpyHostToDevice, e->stream));
  if (olvq)
    hipLaunchKernelGGL(k_lvq_amax, dim3(1), dim3(256), 0, e->stream, dev_keys, count * LVQ_K0, dev_ta, p->alpha, b.amax_dev);
  HIPCHK(hipGetLastError());
  int done = 0, reason = 0;
  int64_t nmod = 0;
  CHK(lvq_walk_batch(cb, ds, b, (const LvqStep *)dst, row0, (int)count, knn, dev_keys, dev_lab, olvq ? dev_ta : (const float *)nullptr,
                     reinterpret_cast<const float4 *>(dev_rows), xrows, olvq ? 0.0f : lvq_amax_of(hst.data(), (int)count), olvq,
                     (uint64_t *)dfin, &done, &reason, &nmod));
  if (done <= 0) return fail("somhip_lvq_batch_apply: batch made no progress (reason %d)", reason);
  if (trace_index || trace_diff) {
    std::vector<uint64_t> hfin((size_t)done * 2);
    HIPCHK(hipMemcpy(hfin.data(), dfin, sizeof(uint64_t) * 2 * (size_t)done, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < done; j++)
      for (int k = 0; k < knn; k++) {
        int32_t idx; float df;
        decode_key(hfin[(size_t)(2 * j + k)], knn == 2, &idx, &df);
        if (trace_index) trace_index[j * knn + k] = idx;
        if (trace_diff) trace_diff[j * knn + k] = df;
      }
  }
  if (reason == 1) e->lvq_stop_list++;
  if (reason == 2) e->lvq_stop_cache++;
  e->lvq_batches++;
  e->lvq_samples += (uint64_t)done;
  *consumed = done;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_lvq_batch_apply)
