// host_quality.inc -- map quality: topographic error, hits and error sum per unit (K1q) behind a top-2 search, and the
// pairs of that search into a pair table (K1c, host_conn.inc)
// (included by somhip.hip: one translation unit, shared static helpers)

// The driver of somhip_map_quality (c null) and somhip_map_connectivity (c the table; out null: the pairs alone), after
// check_pair and the entry point's own null tests; `who` names the entry point in every message.
// K1q (include/somhip.h).  Per chunk (knn_chunk_keys with knn 2 under SOMHIP_TIE_FIRST, so the routes, the chunks, the
// row wrap and masked data are the top-K search's): the keys, k_quality_pairs behind them, k_quality_units behind that,
// one copy of 4 bytes per sample -- the winners' distances, which find_qerror's float chain (som_rout.c:715) then takes
// on the host in data order, where the qerror tool runs it.  hits, qsum and the totals stay on the device for the call.
// K1c: k_conn_keys behind the same keys; the table takes every full slab and what the run ends with.
static int quality_run(const char *who, somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, uint32_t *hits, double *qsum,
                       float qerror_in, somhip_quality_totals *out, somhip_conn *c) {
  if (is_shard(cb)) return fail("%s: sharded codebook not supported (a shard does not hold the other shards' units)", who);
  if (out && ((cb->v.topol != SOMHIP_TOPOL_HEXA && cb->v.topol != SOMHIP_TOPOL_RECT) || (int64_t)cb->v.xdim * cb->ydim != cb->v.n))
    return fail("%s: codebook without a lattice (%d x %d units, %lld rows)", who, cb->v.xdim, cb->ydim, (long long)cb->v.n);
  if (first < 0) return fail("%s: first row %lld < 0", who, (long long)first);
  if (count >= (int64_t)1 << 32) return fail("%s: count %lld does not fit the 32-bit hit counts", who, (long long)count);
  if (c) CHK(conn_check_units(c, cb->v.n, who));
  if (out) *out = somhip_quality_totals{0, 0, 0, qerror_in};
  if (count <= 0) return 0;
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  if (ds->d_mask && !ds->d_all_masked) {                                // the device copy of the rows' flags (a data set with
                                                                        // masks has them), when first wanted
    HIPCHK(hipMalloc((void **)&ds->d_all_masked, (size_t)ds->n));
    HIPCHK(hipMemcpy(ds->d_all_masked, ds->all_masked.data(), (size_t)ds->n, hipMemcpyHostToDevice));
  }
  const size_t n = (size_t)cb->v.n;
  const bool per_unit = hits || qsum;
  const bool pairs = c && n >= 2;                                       // (a map of one unit has no second-best unit)
  if (pairs) CHK(conn_begin(c, cb->v.n, count));
  // [qsum: n doubles][the totals][hits: n words]
  double *dq = nullptr;
  unsigned long long *dtot = nullptr;
  uint32_t *dh = nullptr;
  if (out) {
    void *p;
    CHK(engine_scratch(e, SLOT_QUALITY, (sizeof(double) + sizeof(uint32_t)) * n + sizeof(unsigned long long) * QUAL_TOTALS, &p));
    dq = (double *)p;
    dtot = reinterpret_cast<unsigned long long *>(dq + n);
    dh = reinterpret_cast<uint32_t *>(dtot + QUAL_TOTALS);
    HIPCHK(hipMemsetAsync(dtot, 0, sizeof(unsigned long long) * QUAL_TOTALS, e->stream));
    if (qsum) CHK(to_device(e, dq, qsum, n));
    else if (per_unit) HIPCHK(hipMemsetAsync(dq, 0, sizeof(double) * n, e->stream));
    if (hits) CHK(to_device(e, dh, hits, n));
    else if (per_unit) HIPCHK(hipMemsetAsync(dh, 0, sizeof(uint32_t) * n, e->stream));
  }
  float qerror = qerror_in;
  std::vector<float> hd;
  CHK(knn_chunk_keys(cb, ds, first, count, 2, 0, [&](int64_t off, int64_t f, int64_t cnt, const uint64_t *dk, int stride) {
    (void)off;
    if (pairs) CHK(conn_take_chunk(c, cb, ds, f, cnt, dk, stride));
    if (!out) return 0;
    // [term: cnt doubles][unit: cnt words][d1: cnt floats]
    void *q;
    CHK(engine_scratch(e, SLOT_CALL_B, (sizeof(double) + sizeof(uint32_t) + sizeof(float)) * (size_t)cnt, &q));
    double *dterm = (double *)q;
    uint32_t *dunit = reinterpret_cast<uint32_t *>(dterm + cnt);
    float *dd1 = reinterpret_cast<float *>(dunit + cnt);
    CHK(LAUNCH_TIMED(e, KID_QUALITY_PAIRS, k_quality_pairs, dim3((unsigned)((cnt + QUAL_THREADS - 1) / QUAL_THREADS)), dim3(QUAL_THREADS), 0, dk,
        stride, ds->d_all_masked, f, ds->n, cnt, cb->v.n, cb->v.xdim, cb->v.topol, dunit, dd1, dterm, dtot));
    if (per_unit) {
      if (cnt > QUAL_CHUNK) return fail("%s: a chunk of %lld samples, the unit pass sorts %d", who, (long long)cnt, QUAL_CHUNK);
      CHK(LAUNCH_TIMED(e, KID_QUALITY_UNITS, k_quality_units, dim3(1), dim3(QUAL_SORT_THREADS), 0, dunit, dterm, (int)cnt, dh, dq));
    }
    if (hd.empty()) hd.resize((size_t)cnt);                             // (the first chunk is the longest)
    CHK(to_host_sync(e, hd.data(), dd1, (size_t)cnt));
    for (int64_t i = 0; i < cnt; i++) {
      if (sample_is_empty(ds, (f + i) % ds->n)) continue;               // ignore empty vectors, som_rout.c:712
      qerror += sqrt((double)hd[(size_t)i]);                            // float accumulator, :715
    }
    return 0;
  }));
  if (pairs) CHK(conn_flush(c));
  if (!out) return 0;
  unsigned long long tot[QUAL_TOTALS];
  if (hits) CHK(to_host(e, hits, dh, n));
  if (qsum) CHK(to_host(e, qsum, dq, n));
  CHK(to_host_sync(e, tot, dtot, QUAL_TOTALS));
  out->searched = (int64_t)tot[QUAL_SEARCHED];
  out->topo_defined = (int64_t)tot[QUAL_TOPO_DEFINED];
  out->topo_errors = (int64_t)tot[QUAL_TOPO_ERRORS];
  out->qerror = qerror;
  return 0;
}
extern "C" int somhip_map_quality(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, uint32_t *hits,
                                  double *qsum, float qerror_in, somhip_quality_totals *out) try {
  CHK(check_pair(cb, ds, "somhip_map_quality"));
  if (!out) return fail("somhip_map_quality: null output");
  return quality_run("somhip_map_quality", cb, ds, first, count, hits, qsum, qerror_in, out, nullptr);
} ABI_CATCH(somhip_map_quality)
// K1c (include/somhip.h): the call's pairs into the table; with `out`, somhip_map_quality beside them from the same search
extern "C" int somhip_map_connectivity(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t count, somhip_conn *c, uint32_t *hits,
                                       double *qsum, float qerror_in, somhip_quality_totals *out) try {
  CHK(check_pair(cb, ds, "somhip_map_connectivity"));
  if (!c) return fail("somhip_map_connectivity: null handle");
  if (!c->e) return fail("somhip_map_connectivity: the engine of this handle was destroyed");
  if (c->e != cb->e) return fail("somhip_map_connectivity: codebook and pair table belong to different engines");
  if (!out && (hits || qsum)) return fail("somhip_map_connectivity: hits and qsum need the totals (null output)");
  return quality_run("somhip_map_connectivity", cb, ds, first, count, hits, qsum, qerror_in, out, c);
} ABI_CATCH(somhip_map_connectivity)
// HIP-event totals of the two kernels since somhip_timing_reset, while somhip_timing_enable is on (ids of their own behind
// the published table, like the vote's): [0] k_quality_pairs, [1] k_quality_units
extern "C" int somhip_map_quality_timing(somhip_engine *e, int64_t launches[2], double total_ms[2]) try {
  const int kid[2] = {KID_QUALITY_PAIRS, KID_QUALITY_UNITS};
  return stage_timing(e, "somhip_map_quality_timing", kid, 2, launches, total_ms);
} ABI_CATCH(somhip_map_quality_timing)
