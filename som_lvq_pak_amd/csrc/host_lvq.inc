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

// Every choice of one somhip_lvq_train call or one somhip_lvq_batch_apply, made here and nowhere else (reported by
// somhip_debug_lvq_plan).  Made per call, never kept on the engine: the switches may change between two calls.
//   SOMHIP_LVQ_ONLINE=1      the one-launch-per-iteration engine even where the batched one fits
//   SOMHIP_LVQ_SYNC=1        every batch the careful way (its verdict read back before the next is launched)
//   SOMHIP_LVQ_SERIAL=1      every batch one component (the serial walk), the careful way
//   SOMHIP_LVQ_PAIRS_VALU=1  relation (*) always by the direct-form kernel
enum { LVQ_PAIRS_MASKED = 0, LVQ_PAIRS_MFMA = 1, LVQ_PAIRS_DIRECT = 2 };
struct LvqPlan {
  bool fits;       // row-ordered codebook whose rows fit the walk's on-chip cache: the batched engine can run it
  bool batched;    // somhip_lvq_train: the exact batched engine (else one k_lvq_online_step launch per iteration)
  bool nowait;     // its loop launches batch after batch without waiting for the host (else every batch the careful way)
  bool single;     // the whole batch is one component
  int pairs;       // relation (*) over all pairs: LVQ_PAIRS_MASKED direct form over the components both samples have,
                   // LVQ_PAIRS_MFMA Gram form on the matrix pipe (dim % 8 == 0), LVQ_PAIRS_DIRECT direct form
  bool masked, olvq;
  int knn;         // winners per sample: 2 for LVQ2.1 / LVQ3, else 1
  int slots;       // rows the walk's cache holds
  size_t dyn;      // ... and its dynamic LDS bytes
};
static LvqPlan lvq_plan(const somhip_codebook *cb, const somhip_dataset *ds, const somhip_lvq_params *p, bool want_trace) {
  LvqPlan pl;
  pl.slots = lvq_cache_slots(cb->v.d4);
  pl.dyn = ((size_t)cb->v.d4 * pl.slots + 3 * (size_t)cb->v.d4) * sizeof(float4);
  pl.fits = cb->v.patch_w == 0 && cb->v.d4 <= LVQ_BT && pl.slots >= 8;
  pl.batched = pl.fits && !getenv("SOMHIP_LVQ_ONLINE");
  pl.single = getenv("SOMHIP_LVQ_SERIAL") != nullptr;
  // no waiting only if the winners of the whole call fit a device buffer (they are read back at the end)
  pl.nowait = !getenv("SOMHIP_LVQ_SYNC") && !pl.single && (!want_trace || p->count <= (1ll << 22));
  pl.masked = ds->d_mask != nullptr;
  pl.pairs = pl.masked ? LVQ_PAIRS_MASKED : ds->d % 8 == 0 && !getenv("SOMHIP_LVQ_PAIRS_VALU") ? LVQ_PAIRS_MFMA : LVQ_PAIRS_DIRECT;
  pl.olvq = p->kind == SOMHIP_OLVQ1;
  pl.knn = p->kind >= SOMHIP_LVQ2 ? 2 : 1;
  return pl;
}
// the plan of a somhip_lvq_train call with these arguments (somhip.h): host arithmetic only
extern "C" int somhip_debug_lvq_plan(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p, int want_trace,
                                     int32_t *out) try {
  CHK(check_pair(cb, ds, "somhip_debug_lvq_plan"));
  if (!p || !out) return fail("somhip_debug_lvq_plan: null argument");
  if (p->kind < SOMHIP_LVQ1 || p->kind > SOMHIP_LVQ3) return fail("Unknown LVQ type %d", p->kind);
  const LvqPlan pl = lvq_plan(cb, ds, p, want_trace != 0);
  out[0] = pl.batched; out[1] = pl.nowait; out[2] = pl.single; out[3] = pl.pairs;
  out[4] = pl.masked; out[5] = pl.knn; out[6] = pl.slots; out[7] = (int32_t)pl.dyn;
  return 0;
} ABI_CATCH(somhip_debug_lvq_plan)

// device buffers of one batch of the exact LVQ engine
struct LvqBatchBufs {
  float *rho, *xnorm; uint32_t *adj; int32_t *comp_samples; LvqBatchOut *out;
  float4 *stage_rows; int32_t *stage_rowid; float *stage_ta;
  int32_t *cand_lab; float *cand_ta; int32_t *mod_rows, *mod_count; float *amax_dev;
};
// one batch after its candidate lists are known: data rows [row0, row0 + c) (mod n)
struct LvqBatch {
  int64_t row0; int c;
  const LvqStep *st;               // device: the step scalars [c]
  const uint64_t *cand;            // device: global top-8 keys [c][8]
  const int32_t *lab;              // ... the candidates' labels
  const float *ta;                 // ... and OLVQ1 rates (else nullptr)
  const float4 *xrows; int xc;     // sharded codebooks only: tile copies [c][xc][d4] of the xc nearest candidates
  float amax;                      // bound on |rate| of every correction of the batch (< 0 -- a NaN in the schedule --:
                                   // unknown, and k_lvq_sample_rho makes the whole batch one component) ...
  const float *amax_dev;           // ... or, if not null, where the device holds it (OLVQ1: lvq_rate_bound)
  uint64_t *fin;                   // device: where the batch's winners go (trace)
};

// the engine's scratch slots behind LvqBatchBufs; the first use on an engine also raises two kernels' dynamic LDS limit
static int lvq_batch_bufs(somhip_engine *e, int d4, LvqBatchBufs *b) {
  CHK(scratch(e, SLOT_LVQ_RHO, (size_t)2 * LVQ_BMAX + 4, &b->rho)); b->xnorm = b->rho + LVQ_BMAX; b->amax_dev = b->xnorm + LVQ_BMAX;
  CHK(scratch(e, SLOT_LVQ_ADJ, (size_t)LVQ_BMAX * LVQ_AW, &b->adj));
  CHK(scratch(e, SLOT_LVQ_COMP, (size_t)LVQ_BMAX, &b->comp_samples));
  CHK(scratch(e, SLOT_LVQ_OUT, 1, &b->out));
  CHK(scratch(e, SLOT_LVQ_STAGE_ROWS, 2 * LVQ_BMAX * (size_t)d4, &b->stage_rows));
  CHK(scratch(e, SLOT_LVQ_STAGE_ROWID, (size_t)2 * LVQ_BMAX, &b->stage_rowid));
  CHK(scratch(e, SLOT_LVQ_STAGE_TA, (size_t)2 * LVQ_BMAX, &b->stage_ta));
  CHK(scratch(e, SLOT_LVQ_CAND_LAB, (size_t)LVQ_BMAX * LVQ_K0, &b->cand_lab));
  CHK(scratch(e, SLOT_LVQ_CAND_TA, (size_t)LVQ_BMAX * LVQ_K0, &b->cand_ta));
  CHK(scratch(e, SLOT_LVQ_MOD, (size_t)2 * LVQ_BMAX + 4, &b->mod_rows)); b->mod_count = b->mod_rows + 2 * LVQ_BMAX;
  // the walk's row cache and the component kernel's adjacency rows need more dynamic LDS than the default limit
  CHK(raise_lds_limit(e, LDS_LVQ_APPLY, (const void *)k_lvq_batch_apply<false>, LVQ_DYN_LDS));
  CHK(raise_lds_limit(e, LDS_LVQ_APPLY_MASKED, (const void *)k_lvq_batch_apply<true>, LVQ_DYN_LDS));
  return raise_lds_limit(e, LDS_LVQ_COMPONENTS, (const void *)k_lvq_components, LVQ_BMAX * LVQ_AW * 4);
}

// ---- small jobs every LVQ entry point shares --------------------------------------------------------------------
// the step scalars of iterations [it0, it0 + c) on data rows row0, row0 + 1, ... (mod n)
static void lvq_fill_steps(const somhip_dataset *ds, const somhip_lvq_params *p, int64_t it0, int64_t row0, int64_t c, LvqStep *st) {
  const float ratio = (1 - p->winlen) / (1 + p->winlen);                  // lvq_rout.c:770, fp32
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
}
// bound on |rate| of the batch's corrections from its step scalars (LVQ1 / LVQ2.1 / LVQ3: the schedule value, and
// alpha * epsilon); OLVQ1 rates live per row: see lvq_rate_bound
static float lvq_amax_of(const LvqStep *st, int c) {
  float m = 0.0f;
  for (int j = 0; j < c; j++) {
    const float a = std::fabs(st[j].alpha), ae = std::fabs(st[j].alpha * st[j].epsilon);
    if (!(a == a) || !(ae == ae)) return -1.0f;
    m = std::max(m, std::max(a, ae));
  }
  return m;
}
// the winner trace of iterations [it0, it0 + c) from their keys [c][2] (host)
static void lvq_trace(const uint64_t *keys, int64_t c, int knn, int64_t it0, int32_t *trace_index, float *trace_diff) {
  for (int64_t j = 0; j < c; j++)
    for (int k = 0; k < knn; k++) {
      int32_t idx; float df;
      decode_key(keys[(size_t)(2 * j + k)], knn == 2, &idx, &df);
      if (trace_index) trace_index[(it0 + j) * knn + k] = idx;
      if (trace_diff) trace_diff[(it0 + j) * knn + k] = df;
    }
}
// ... from keys on the device, of walks the host has already waited for
static int lvq_trace_read(const uint64_t *d_keys, int64_t c, int knn, int64_t it0, int32_t *trace_index, float *trace_diff) {
  std::vector<uint64_t> hfin((size_t)c * 2);
  HIPCHK(hipMemcpy(hfin.data(), d_keys, sizeof(uint64_t) * 2 * (size_t)c, hipMemcpyDeviceToHost));
  lvq_trace(hfin.data(), c, knn, it0, trace_index, trace_diff);
  return 0;
}
// masked data: a sample with every component masked has no winner, and the reference then adapts through a NULL
// winner (lvq_rout.c:542-545) -- refuse a run over such a row before anything is trained
static int lvq_refuse_all_masked(const somhip_dataset *ds, int64_t data_first, int64_t count, const char *who) {
  if (!ds->d_mask) return 0;
  for (int64_t j = 0; j < std::min<int64_t>(count, ds->n); j++) {
    const int64_t r = (data_first + j) % ds->n;
    if (sample_is_empty(ds, r))
      return fail("%s: data row %lld has every component masked: no winner (the reference crashes here)", who, (long long)r);
  }
  return 0;
}
// OLVQ1's per-row rates to the device and back, on the engine's stream (the caller waits)
static int lvq_rates_to_device(somhip_codebook *cb, const float *talpha) {
  if (!cb->d_talpha) HIPCHK(hipMalloc((void **)&cb->d_talpha, sizeof(float) * (size_t)cb->v.n));
  return to_device(cb->e, cb->d_talpha, talpha, (size_t)cb->v.n);
}
static int lvq_rates_to_host(somhip_codebook *cb, float *talpha) {
  return to_host(cb->e, talpha, cb->d_talpha, (size_t)cb->v.n);
}

// ---- the stages of one batch (kernels/lvq_batch.hpp), each launched from here only ----------------------------------
// front: labels and (OLVQ1; ta may be null otherwise) rates of the listed rows ...
static int lvq_cand_meta(somhip_codebook *cb, const uint64_t *d_keys, int64_t count, int knn, bool olvq, int32_t *d_lab, float *d_ta) {
  return LAUNCH(cb->e, k_lvq_cand_meta, dim3((unsigned)((count * LVQ_K0 + 255) / 256)), dim3(256), 0, cb->v, d_keys, count * LVQ_K0, knn,
                cb->d_labels, olvq ? cb->d_talpha : nullptr, d_lab, d_ta);
}
// ... and OLVQ1's bound on |rate| of the batch's corrections, from the listed rows' rates
static int lvq_rate_bound(somhip_engine *e, const uint64_t *d_keys, int64_t count, const float *d_ta, float clamp, float *amax_dev) {
  return LAUNCH(e, k_lvq_amax, dim3(1), dim3(256), 0, d_keys, count * LVQ_K0, d_ta, clamp, amax_dev);
}

// pairs: rho_j of relation (*) for every sample (masked data: the sample's norm over its own components), then the
// relation over all pairs of the batch by the plan's kernel
static int lvq_pairs(somhip_engine *e, somhip_dataset *ds, const LvqPlan &pl, const LvqBatchBufs &b, const LvqBatch &bt) {
  const unsigned nt = (unsigned)((bt.c + 63) / 64);
  CHK((with_value<1, 0>(pl.masked, [&](auto m) {
    return LAUNCH(e, k_lvq_sample_rho<decltype(m)::value != 0>, dim3((unsigned)((bt.c + 3) / 4)), dim3(256), 0, ds->d_rows, ds->n, ds->d, bt.row0, bt.c,
                  bt.cand, bt.amax, bt.amax_dev, b.rho, b.xnorm, ds->d_mask);
  })));
  if (pl.pairs == LVQ_PAIRS_MFMA)
    return LAUNCH(e, k_lvq_pair_adj_mfma, dim3(nt, nt), dim3(256), 0, ds->d_rows, ds->n, ds->d, bt.row0, bt.c, b.rho, b.xnorm, b.adj);
  return with_value<1, 0>(pl.masked, [&](auto m) {
    return LAUNCH(e, k_lvq_pair_adj<decltype(m)::value != 0>, dim3(nt, nt), dim3(256), 0, ds->d_rows, ds->n, ds->d, bt.row0, bt.c, b.rho, b.adj,
                  ds->d_mask);
  });
}
// components: the connected components of the adjacency rows of c samples (single: one component, the rows unread)
static int lvq_components(somhip_engine *e, const LvqBatchBufs &b, int c, bool single) {
  return LAUNCH(e, k_lvq_components, dim3(1), dim3(LVQ_BMAX), (size_t)c * LVQ_AW * 4, b.adj, c, single ? 1 : 0, b.comp_samples, b.out);
}
// relation: the pairs stage (unless the plan makes the batch one component) and the components stage
static int lvq_relation(somhip_engine *e, somhip_dataset *ds, const LvqPlan &pl, const LvqBatchBufs &b, const LvqBatch &bt) {
  LaunchTimer t(e, KID_LVQ_COMPONENTS);
  if (!pl.single) CHK(lvq_pairs(e, ds, pl, b, bt));
  return lvq_components(e, b, bt.c, pl.single);
}

// walk: one workgroup per component walks its samples < limit in order (k_lvq_batch_apply<true> stages the sample's
// mask row beside the sample)
static int lvq_walk(somhip_codebook *cb, somhip_dataset *ds, const LvqPlan &pl, const LvqBatchBufs &b, const LvqBatch &bt, int limit) {
  somhip_engine *e = cb->e;
  return with_value<1, 0>(pl.masked, [&](auto m) {
    return LAUNCH_TIMED(e, KID_LVQ_BATCH_APPLY, k_lvq_batch_apply<decltype(m)::value != 0>, dim3((unsigned)bt.c), dim3(LVQ_BT), pl.dyn, cb->v, ds->d_rows,
                        ds->n, bt.row0, limit, bt.lab, bt.ta, bt.xrows, bt.xc, bt.cand, bt.st, pl.knn, pl.slots, b.comp_samples, bt.fin, b.stage_rows,
                        b.stage_rowid, b.stage_ta, b.out, ds->d_mask);
  });
}

// commit: the staged rows (OLVQ1: rates) of ncomp components into the rows this shard owns, with the list of rows it
// wrote; with a control block, only if every component ran through and no earlier batch was left stopped
static int lvq_commit(somhip_codebook *cb, const LvqPlan &pl, const LvqBatchBufs &b, const LvqBatch &bt, int ncomp, LvqCtl *d_ctl,
                      int batch_id) {
  somhip_engine *e = cb->e;
  HIPCHK(hipMemsetAsync(b.mod_count, 0, sizeof(int32_t), e->stream));
  return LAUNCH_TIMED(e, KID_LVQ_BATCH_APPLY, k_lvq_commit, dim3((unsigned)ncomp), dim3(256), 0, cb->v, b.out, b.stage_rows, b.stage_rowid, b.stage_ta,
                      pl.knn == 1 && bt.ta ? cb->d_talpha : nullptr, b.mod_rows, b.mod_count, d_ctl, batch_id, d_ctl ? bt.c : 0);
}

// refresh of prepared rows: the bf16 copies / norms of exactly the rows this batch corrected (at most `bound` of them;
// none if *skip), so that the next batch's pre-filter (big codebooks, scan_keys_topk) needs no pass over the whole
// codebook -- only if they were current for the codebook this batch started from (a scan that took the direct path
// never made them so: re-splitting a few rows of stale tiles must not validate them)
static int lvq_refresh_prepared(somhip_codebook *cb, const LvqBatchBufs &b, int bound, const int32_t *skip) {
  somhip_engine *e = cb->e;
  if (!cb->prep_valid || !cb->d_chi || !cb->d_cn || e->scan_mode != SOMHIP_SCAN_MFMA_BF16) { rows_written(cb); return 0; }
  close_accumulations(cb);                                              // (rows were rewritten: an accumulation no longer describes them)
  CHK(LAUNCH(e, k_prep_rows_bf16, dim3((unsigned)((bound + 3) / 4)), dim3(256), 0, cb->v, (cb->v.d4 + 1) / 2, b.mod_rows, bound, b.mod_count,
      cb->d_cn, cb->d_chi, cb->d_clo, skip));
  cb->rowmajor_valid = false;                             // (the row-major copy is not re-split row by row)
  return 0;
}

// One batch the careful way: relation (*) -> components -> one workgroup per component walks its samples in order ->
// (repeat with the batch cut at the first stop, if any) -> commit -> refresh.  *consumed <= bt.c samples were applied;
// *reason: why the batch was cut (0: it was not).
static int lvq_batch_careful(somhip_codebook *cb, somhip_dataset *ds, const LvqPlan &pl, const LvqBatchBufs &b, const LvqBatch &bt,
                             int *consumed, int *reason) {
  somhip_engine *e = cb->e;
  CHK(lvq_relation(e, ds, pl, b, bt));
  static_assert(sizeof(LvqBatchOut) < 32768, "summary block");
  std::vector<char> hbuf(sizeof(LvqBatchOut));
  LvqBatchOut *ho = reinterpret_cast<LvqBatchOut *>(hbuf.data());
  int limit = bt.c;
  for (int pass = 0; pass < 2; pass++) {
    CHK(lvq_walk(cb, ds, pl, b, bt, limit));
    CHK(to_host_sync(e, ho, b.out, 1));
    if (ho->ncomp < 1 || ho->ncomp > bt.c) return fail("somhip_lvq_train: bad component count %d", ho->ncomp);
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
  int bound = 0, big = 0;
  for (int k = 0; k < ho->ncomp; k++) {
    bound += ho->nslots[k];
    big = std::max(big, ho->start[k + 1] - ho->start[k]);
  }
  e->lvq_components += (uint64_t)ho->ncomp;
  e->lvq_largest += (uint64_t)big;
  for (int k = 0; k < 4; k++) e->lvq_cycles[k] += (uint64_t)ho->cycles[k];
  if (limit > 0 && bound > 0) {
    CHK(lvq_commit(cb, pl, b, bt, ho->ncomp, nullptr, 0));
    CHK(lvq_refresh_prepared(cb, b, bound, nullptr));
  }
  return 0;
}

// One batch as the loop below launches it when it does not wait for the host: relation (*), components, one walk
// over the whole batch, then a commit that happens only if every component ran through (the control block) and a
// refresh that is skipped if it did not -- no read-back in between.  At most two rows per sample are corrected.
static int lvq_batch_nowait(somhip_codebook *cb, somhip_dataset *ds, const LvqPlan &pl, const LvqBatchBufs &b, const LvqBatch &bt,
                            LvqCtl *d_ctl, int batch_id) {
  CHK(lvq_relation(cb->e, ds, pl, b, bt));
  CHK(lvq_walk(cb, ds, pl, b, bt, bt.c));
  CHK(lvq_commit(cb, pl, b, bt, bt.c, d_ctl, batch_id));
  return lvq_refresh_prepared(cb, b, 2 * bt.c, (const int32_t *)&d_ctl->poison);
}

// The exact batched engine's loop.  Batch after batch is launched without waiting for the one before (its scalars
// go through the ring of pinned buffers, its verdict stays on the device: LvqCtl); the control block of every batch
// is read back asynchronously and looked at a few batches later.  A batch that stopped early -- rare: the candidate
// lists and the row cache are sized so that it is -- has poisoned everything launched after it; the host then redoes
// that one batch with lvq_batch_careful (which cuts it at the stop and reads the verdict back) and goes on from there.
// A plan without nowait: every batch the careful way.
static int lvq_train_batched(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p, const LvqPlan &pl,
                             int32_t *trace_index, float *trace_diff) {
  somhip_engine *e = cb->e;
  const int64_t BMAX = LVQ_BMAX;
  constexpr int RING = LVQ_EV_RING;
  uint64_t *dcand, *dfin; LvqStep *dst; LvqCtl *dctl;
  const bool want_trace = trace_index || trace_diff;
  const bool nowait = pl.nowait;
  CHK(scratch(e, SLOT_CALL_A, (size_t)BMAX * LVQ_K0, &dcand));
  CHK(scratch(e, SLOT_CALL_B, (size_t)BMAX, &dst));
  CHK(scratch(e, SLOT_LVQ_FINAL, 2 * (size_t)(nowait && want_trace ? std::max<int64_t>(p->count, BMAX) : BMAX), &dfin));
  CHK(scratch(e, SLOT_LVQ_CTL, 1, &dctl));
  LvqBatchBufs b;
  CHK(lvq_batch_bufs(e, cb->v.d4, &b));
  if (!e->lvq_hctl) HIPCHK(hipHostMalloc((void **)&e->lvq_hctl, sizeof(LvqCtl) * RING, hipHostMallocDefault));
  for (int i = 0; i < RING; i++)
    if (!e->lvq_ev[i]) HIPCHK(hipEventCreateWithFlags(&e->lvq_ev[i], hipEventDisableTiming));
  HIPCHK(hipMemsetAsync(dctl, 0, sizeof(LvqCtl), e->stream));
  std::vector<LvqStep> hst((size_t)BMAX);
  int64_t B = std::max<int64_t>(32, std::min<int64_t>(BMAX, e->lvq_batch_hint));   // what the previous call ended with
  int64_t off = 0;
  uint64_t n_sync_batches = 0;
  // the c samples from offset o of the call: their step scalars (host, on their way to dst already) -> the front
  // (candidate lists, their labels / rates, the OLVQ1 rate bound) -> the batch
  auto front = [&](int64_t o, int64_t c, const LvqStep *st, uint64_t *fin, LvqBatch *bt) -> int {
    const int64_t row0 = (p->data_first + o) % ds->n;
    float *ta = pl.olvq ? b.cand_ta : (float *)nullptr;
    CHK(scan_keys_topk<LVQ_K0>(cb, ds, row0, c, dcand, pl.knn == 2 ? 1 : 0));
    CHK(lvq_cand_meta(cb, (const uint64_t *)dcand, c, pl.knn, pl.olvq, b.cand_lab, ta));
    if (pl.olvq) CHK(lvq_rate_bound(e, (const uint64_t *)dcand, c, ta, p->alpha, b.amax_dev));
    *bt = {row0, (int)c, (const LvqStep *)dst, (const uint64_t *)dcand, b.cand_lab, ta, nullptr, 0,
           pl.olvq ? 0.0f : lvq_amax_of(st, (int)c), pl.olvq ? b.amax_dev : (float *)nullptr, fin};
    return 0;
  };
  struct Pending { int64_t off, c; int id; };
  Pending ring[RING];
  int head = 0, tail = 0, next_id = 1;                    // batches in flight: ring[tail % RING .. head % RING)
  int64_t launched = 0;                                   // samples launched so far (assuming every batch runs through)
  LvqBatch bt;
  while (off < p->count) {
    if (nowait) {
      // ---- keep launching; look at the oldest read-back when the ring is full or nothing is left to launch
      if (launched < p->count && head - tail < RING) {
        const int64_t c = std::min(B, p->count - launched);
        void *hv; int slot;
        CHK(pin_acquire(e, sizeof(LvqStep) * (size_t)c, &hv, &slot));
        lvq_fill_steps(ds, p, p->start_iter + launched, p->data_first + launched, c, (LvqStep *)hv);
        CHK(pin_upload(e, slot, dst, (size_t)c));
        CHK(front(launched, c, (const LvqStep *)hv, dfin + (want_trace ? 2 * launched : 0), &bt));
        const int id = next_id++;
        CHK(lvq_batch_nowait(cb, ds, pl, b, bt, dctl, id));
        CHK(to_host(e, &e->lvq_hctl[head % RING], dctl, 1));
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
    // ---- one batch the careful way (a plan without nowait, or the redo of a batch that stopped early)
    const int64_t c = std::min(B, p->count - off);
    lvq_fill_steps(ds, p, p->start_iter + off, p->data_first + off, c, hst.data());
    CHK(to_device(e, dst, hst.data(), (size_t)c));
    CHK(front(off, c, hst.data(), dfin + (nowait && want_trace ? 2 * off : 0), &bt));
    int consumed = 0, reason = 0;
    CHK(lvq_batch_careful(cb, ds, pl, b, bt, &consumed, &reason));
    if (consumed <= 0)
      // cannot happen: with an empty cache every winner comes from the frozen list and one or two slots always fit
      return fail("somhip_lvq_train: batch made no progress (reason %d)", reason);
    if (want_trace && !nowait) CHK(lvq_trace_read((const uint64_t *)dfin, consumed, pl.knn, off, trace_index, trace_diff));
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
  CHK(to_host_sync(e, &fin_ctl, dctl, 1));
  if (fin_ctl.poison) return fail("somhip_lvq_train: a stopped batch was left behind (batch %d)", fin_ctl.batch);
  e->lvq_components += fin_ctl.comps;
  e->lvq_largest += fin_ctl.largest;
  for (int k = 0; k < 4; k++) e->lvq_cycles[k] += fin_ctl.cycles[k];
  if (nowait && want_trace) CHK(lvq_trace_read((const uint64_t *)dfin, p->count, pl.knn, 0, trace_index, trace_diff));
  e->lvq_batches += n_sync_batches + fin_ctl.batches;
  e->lvq_samples += (uint64_t)p->count;
  e->lvq_batch_hint = B;
  return 0;
}

// The one-launch-per-iteration engine: k_lvq_online_step applies the previous iteration's correction and searches
// the current sample's winners in one pass over the codebook.
static int lvq_train_online(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p, const LvqPlan &pl,
                            int32_t *trace_index, float *trace_diff) {
  somhip_engine *e = cb->e;
  rows_written(cb);            // the per-iteration kernel rewrites rows in place
  const int64_t CH = 4096;
  const int nblk = (int)((cb->v.ngroups + 3) / 4);
  const bool want_trace = trace_index || trace_diff;
  uint64_t *dpart, *fin; LvqStep *st;
  CHK(scratch(e, SLOT_PARTIAL, (size_t)nblk * 2 * 2, &dpart));
  CHK(scratch(e, SLOT_CALL_A, (size_t)(CH + 1) * 2, &fin));
  CHK(scratch(e, SLOT_CALL_B, (size_t)(CH + 1), &st));
  uint64_t *part[2] = {dpart, dpart + (size_t)nblk * 2};
  std::vector<LvqStep> hst((size_t)CH + 1);
  std::vector<uint64_t> hfin((size_t)(CH + 1) * 2);
  int64_t prev_row = 0;
  bool have_prev = false;
  int flip = 0;
  // one iteration: the correction of the sample before (if any) with its scalars st_j, the winners of data row cur_row
  // (if has_cur); the merged winners of the sample before go to fin_j
  auto step = [&](int64_t cur_row, int has_cur, uint64_t *fin_j, const LvqStep *st_j) -> int {
    CHK((with_value<1, 0>(pl.masked, [&](auto m) {
      return LAUNCH_TIMED(e, KID_LVQ_ONLINE_STEP, k_lvq_online_step<decltype(m)::value != 0>, dim3((unsigned)nblk), dim3(256), 0, cb->v, ds->d_rows,
                          ds->d_mask, cb->d_labels, cb->d_talpha, prev_row, cur_row, have_prev ? 1 : 0, has_cur, pl.knn, part[flip], nblk,
                          part[flip ^ 1], fin_j, st_j);
    })));
    flip ^= 1;
    prev_row = cur_row;
    have_prev = true;
    return 0;
  };
  // fin[j] receives the merged winners of chunk-iteration j-1 when iteration j launches;
  // the last one of a chunk lands in fin[c] when the next chunk's first launch (or the
  // flush) runs, so traces are read one launch late.
  for (int64_t off = 0; off < p->count; off += CH) {
    const int64_t c = std::min(CH, p->count - off);
    const int64_t row0 = (p->data_first + off) % ds->n;
    lvq_fill_steps(ds, p, p->start_iter + off, row0, c, hst.data() + 1);
    CHK(to_device(e, st + 1, hst.data() + 1, (size_t)c));
    for (int64_t j = 0; j < c; j++) CHK(step((row0 + j) % ds->n, 1, fin + 2 * j, st + j));
    // winners of iterations (off-1 .. off+c-2) are now in fin[0..c-1]; fin[0] of the first chunk holds nothing
    if (want_trace) {
      CHK(to_host_sync(e, hfin.data(), fin, 2 * (size_t)c));
      const int64_t skip = off == 0 ? 1 : 0;
      lvq_trace(hfin.data() + 2 * skip, c - skip, pl.knn, off - 1 + skip, trace_index, trace_diff);
    }
    CHK(on_device(e, st, st + c, 1));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  // flush: apply the last iteration's correction; its winners land in fin[0]
  CHK(step(prev_row, 0, fin, st));
  if (want_trace) {
    CHK(to_host_sync(e, hfin.data(), fin, 2));
    lvq_trace(hfin.data(), 1, pl.knn, p->count - 1, trace_index, trace_diff);
  }
  return 0;
}

// lvq*_training (include/somhip.h): checks, the plan, the engine it names -- the exact batched engine, masked data
// included (the sample's mask in the frozen scan, in relation (*) and in the walk); else (asked for, a patch-ordered
// codebook, a row too long for the cache) one k_lvq_online_step launch per iteration
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
  CHK(lvq_refuse_all_masked(ds, p->data_first, p->count, "somhip_lvq_train"));
  if (is_shard(cb)) return fail("somhip_lvq_train: sharded codebook not supported");
  const LvqPlan pl = lvq_plan(cb, ds, p, trace_index || trace_diff);
  if (pl.knn == 2 && cb->v.n < 2) return fail("somhip_lvq_train: LVQ2/LVQ3 need at least two code rows");
  if (p->count == 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  if (pl.olvq) CHK(lvq_rates_to_device(cb, talpha));
  CHK(pl.batched ? lvq_train_batched(cb, ds, p, pl, trace_index, trace_diff)
                 : lvq_train_online(cb, ds, p, pl, trace_index, trace_diff));
  if (pl.olvq) CHK(lvq_rates_to_host(cb, talpha));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_lvq_train)

// diagnostics (include/somhip.h): one batch's front and relation exactly as lvq_train_batched makes them, under the plan
// of the current environment, through the stage functions above; nothing is walked or committed
static int lvq_read_components(somhip_engine *e, const LvqBatchBufs &b, int count, int32_t *ncomp, int32_t *start,
                               int32_t *comp_samples) {
  std::vector<char> hbuf(sizeof(LvqBatchOut));
  LvqBatchOut *ho = reinterpret_cast<LvqBatchOut *>(hbuf.data());
  CHK(to_host(e, ho, b.out, 1));
  CHK(to_host_sync(e, comp_samples, b.comp_samples, (size_t)count));
  *ncomp = ho->ncomp;
  const int nc = std::max(0, std::min(ho->ncomp, count));  // (a wrong count is the caller's finding; read inside the block)
  for (int k = 0; k <= count; k++) start[k] = k <= nc ? ho->start[k] : -1;
  return 0;
}
extern "C" int somhip_debug_lvq_relation(somhip_codebook *cb, somhip_dataset *ds, const somhip_lvq_params *p, int64_t data_first,
                                         int64_t count, uint64_t *keys, float *rho, float *xnorm, float *amax, uint32_t *adj,
                                         int32_t *ncomp, int32_t *start, int32_t *comp_samples) try {
  CHK(check_pair(cb, ds, "somhip_debug_lvq_relation"));
  if (!p || !keys || !rho || !xnorm || !amax || !adj || !ncomp || !start || !comp_samples)
    return fail("somhip_debug_lvq_relation: null argument");
  if (p->kind < SOMHIP_LVQ1 || p->kind > SOMHIP_LVQ3) return fail("Unknown LVQ type %d", p->kind);
  if (count < 1 || count > LVQ_BMAX) return fail("somhip_debug_lvq_relation: a batch has 1..%d samples, not %lld", LVQ_BMAX, (long long)count);
  if (!cb->d_labels) return fail("somhip_debug_lvq_relation: codebook has no labels");
  if (ds->labels.empty()) return fail("somhip_debug_lvq_relation: data has no labels");
  if (data_first < 0) return fail("somhip_debug_lvq_relation: data_first %lld < 0", (long long)data_first);
  if (p->length <= 0 || p->start_iter < 0 || p->start_iter + count > p->length)
    return fail("somhip_debug_lvq_relation: iterations outside schedule");
  if (p->kind == SOMHIP_OLVQ1 && !cb->d_talpha) return fail("somhip_debug_lvq_relation: OLVQ1 needs rates (somhip_lvq_rates_upload)");
  if (is_shard(cb)) return fail("somhip_debug_lvq_relation: sharded codebook not supported");
  CHK(lvq_refuse_all_masked(ds, data_first, count, "somhip_debug_lvq_relation"));
  const LvqPlan pl = lvq_plan(cb, ds, p, false);
  if (!pl.batched)
    return fail("somhip_debug_lvq_relation: this plan does not run the batched engine (%d components per row, SOMHIP_LVQ_ONLINE)", cb->v.d);
  if (pl.knn == 2 && cb->v.n < 2) return fail("somhip_debug_lvq_relation: LVQ2/LVQ3 need at least two code rows");
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  uint64_t *dcand;
  CHK(scratch(e, SLOT_CALL_A, (size_t)LVQ_BMAX * LVQ_K0, &dcand));
  LvqBatchBufs b;
  CHK(lvq_batch_bufs(e, cb->v.d4, &b));
  const int c = (int)count;
  const int64_t row0 = data_first % ds->n;
  std::vector<LvqStep> hst((size_t)c);
  lvq_fill_steps(ds, p, p->start_iter, row0, c, hst.data());
  float *ta = pl.olvq ? b.cand_ta : (float *)nullptr;
  CHK(scan_keys_topk<LVQ_K0>(cb, ds, row0, c, dcand, pl.knn == 2 ? 1 : 0));
  CHK(lvq_cand_meta(cb, (const uint64_t *)dcand, c, pl.knn, pl.olvq, b.cand_lab, ta));
  if (pl.olvq) CHK(lvq_rate_bound(e, (const uint64_t *)dcand, c, ta, p->alpha, b.amax_dev));
  const LvqBatch bt = {row0, c, nullptr, (const uint64_t *)dcand, b.cand_lab, ta, nullptr, 0,
                       pl.olvq ? 0.0f : lvq_amax_of(hst.data(), c), pl.olvq ? b.amax_dev : (float *)nullptr, nullptr};
  CHK(lvq_relation(e, ds, pl, b, bt));
  CHK(to_host(e, keys, dcand, (size_t)c * LVQ_K0));
  *amax = bt.amax;
  if (pl.olvq) CHK(to_host(e, amax, b.amax_dev, 1));
  if (pl.single) {                                        // no pairs stage: nothing of it to report
    std::fill(rho, rho + c, 0.0f);
    std::fill(xnorm, xnorm + c, 0.0f);
    std::fill(adj, adj + (size_t)c * LVQ_AW, 0u);
  } else {
    CHK(to_host(e, rho, b.rho, (size_t)c));
    CHK(to_host(e, xnorm, b.xnorm, (size_t)c));
    CHK(to_host(e, adj, b.adj, (size_t)c * LVQ_AW));
  }
  CHK(lvq_read_components(e, b, c, ncomp, start, comp_samples));
  // words past the batch's last sample belong to no pair: no kernel writes or reads them
  if (!pl.single)
    for (int j = 0; j < c; j++) std::fill(adj + (size_t)j * LVQ_AW + (c + 31) / 32, adj + (size_t)(j + 1) * LVQ_AW, 0u);
  return 0;
} ABI_CATCH(somhip_debug_lvq_relation)
// the components stage alone on adjacency rows the caller made
extern "C" int somhip_debug_lvq_components(somhip_engine *e, const uint32_t *adj, int64_t count, int single, int32_t *ncomp,
                                           int32_t *start, int32_t *comp_samples) try {
  if (!e || !adj || !ncomp || !start || !comp_samples) return fail("somhip_debug_lvq_components: null argument");
  if (count < 1 || count > LVQ_BMAX) return fail("somhip_debug_lvq_components: a batch has 1..%d samples, not %lld", LVQ_BMAX, (long long)count);
  HIPCHK(hipSetDevice(e->device));
  LvqBatchBufs b;
  CHK(lvq_batch_bufs(e, 1, &b));
  CHK(to_device(e, b.adj, adj, (size_t)count * LVQ_AW));
  CHK(lvq_components(e, b, (int)count, single != 0));
  return lvq_read_components(e, b, (int)count, ncomp, start, comp_samples);
} ABI_CATCH(somhip_debug_lvq_components)


// ---------------------------------------------------------------------------------
// lvq*_training over a row-sharded codebook (multi-GPU): one batch in three calls, the host's
// collectives between them (include/somhip.h)
// ---------------------------------------------------------------------------------
extern "C" int somhip_lvq_rates_upload(somhip_codebook *cb, const float *talpha) try {
  CHK(check_codebook(cb, talpha, "somhip_lvq_rates_upload"));
  HIPCHK(hipSetDevice(cb->e->device));
  CHK(lvq_rates_to_device(cb, talpha));
  HIPCHK(hipStreamSynchronize(cb->e->stream));
  return 0;
} ABI_CATCH(somhip_lvq_rates_upload)
extern "C" int somhip_lvq_rates_download(somhip_codebook *cb, float *talpha) try {
  CHK(check_codebook(cb, talpha, "somhip_lvq_rates_download"));
  if (!cb->d_talpha) return fail("somhip_lvq_rates_download: no rates on this codebook");
  HIPCHK(hipSetDevice(cb->e->device));
  CHK(lvq_rates_to_host(cb, talpha));
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
    return LAUNCH(e, k_merge_shard_topk<decltype(k)::value>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, dev_gathered, n_shards, count,
                  dev_keys);
  });
} ABI_CATCH(somhip_merge_topk_keys)
extern "C" int somhip_lvq_batch_candidates(somhip_codebook *cb, int64_t count, int kind, const uint64_t *dev_keys, int xrows,
                                           int32_t *dev_lab, float *dev_ta, float *dev_rows) try {
  CHK(check_codebook(cb, dev_keys && dev_lab && dev_rows, "somhip_lvq_batch_candidates"));
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
  CHK(lvq_cand_meta(cb, dev_keys, count, knn, kind == SOMHIP_OLVQ1, dev_lab, dev_ta));
  return LAUNCH(e, k_lvq_cand_rows, dim3((unsigned)(count * xrows)), dim3(256), 0, cb->v, dev_keys, (int)count, xrows, knn,
                reinterpret_cast<float4 *>(dev_rows));
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
  CHK(lvq_refuse_all_masked(ds, data_first, count, "somhip_lvq_batch_apply"));
  if (xrows < 1 || xrows > LVQ_K0) return fail("somhip_lvq_batch_apply: xrows must be 1..%d", LVQ_K0);
  if (p->kind == SOMHIP_OLVQ1 && (!cb->d_talpha || !dev_ta)) return fail("somhip_lvq_batch_apply: OLVQ1 needs rates (somhip_lvq_rates_upload)");
  const LvqPlan pl = lvq_plan(cb, ds, p, false);          // (one batch, the careful way: the loop's form is the caller's)
  if (!pl.fits)
    return fail("somhip_lvq_batch_apply: rows of %d components do not fit the on-chip cache of the batched engine", cb->v.d);
  *consumed = 0;
  if (count == 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  LvqStep *dst; uint64_t *dfin;
  CHK(scratch(e, SLOT_CALL_B, (size_t)LVQ_BMAX, &dst));
  CHK(scratch(e, SLOT_LVQ_FINAL, (size_t)LVQ_BMAX * 2, &dfin));
  LvqBatchBufs b;
  CHK(lvq_batch_bufs(e, cb->v.d4, &b));
  std::vector<LvqStep> hst((size_t)count);
  const int64_t row0 = data_first % ds->n;
  lvq_fill_steps(ds, p, batch_start_iter, row0, count, hst.data());
  CHK(to_device(e, dst, hst.data(), (size_t)count));
  if (pl.olvq) CHK(lvq_rate_bound(e, dev_keys, count, dev_ta, p->alpha, b.amax_dev));
  const LvqBatch bt = {row0, (int)count, (const LvqStep *)dst, dev_keys, dev_lab, pl.olvq ? dev_ta : (const float *)nullptr,
                       reinterpret_cast<const float4 *>(dev_rows), xrows, pl.olvq ? 0.0f : lvq_amax_of(hst.data(), (int)count),
                       pl.olvq ? b.amax_dev : (float *)nullptr, dfin};
  int done = 0, reason = 0;
  CHK(lvq_batch_careful(cb, ds, pl, b, bt, &done, &reason));
  if (done <= 0) return fail("somhip_lvq_batch_apply: batch made no progress (reason %d)", reason);
  if (trace_index || trace_diff) CHK(lvq_trace_read((const uint64_t *)dfin, done, pl.knn, 0, trace_index, trace_diff));
  if (reason == 1) e->lvq_stop_list++;
  if (reason == 2) e->lvq_stop_cache++;
  e->lvq_batches++;
  e->lvq_samples += (uint64_t)done;
  *consumed = done;
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_lvq_batch_apply)
