// host_class.inc -- within-class nearest later row of a data set (kernels/class_nearest.hpp)
// (part of somhip.hip: same translation unit)

constexpr int CLASS_S = 32;            // later rows per register tile, unmasked (K1's SCAN_S)
constexpr int CLASS_S_MASKED = 16;     // ... masked: every running sum also carries a count of skipped components

// the class segments of n labelled rows: a stable order by label, and for every position the end of its segment
struct ClassOrder {
  std::vector<int32_t> perm;       // [n] position -> row
  std::vector<int32_t> seg_end;    // [groups * 64] position -> one past the last position of its class; 0 in the padding
  int64_t largest = 0;             // rows of the largest class
};
static ClassOrder class_order(const std::vector<int32_t> &labels, int64_t groups) {
  ClassOrder o;
  const int64_t n = (int64_t)labels.size();
  o.perm.resize((size_t)n);
  for (int64_t r = 0; r < n; r++) o.perm[(size_t)r] = (int32_t)r;
  std::stable_sort(o.perm.begin(), o.perm.end(), [&](int32_t a, int32_t b) { return labels[(size_t)a] < labels[(size_t)b]; });
  o.seg_end.assign((size_t)groups * WAVE, 0);
  for (int64_t a = 0; a < n;) {
    int64_t b = a + 1;
    while (b < n && labels[(size_t)o.perm[(size_t)b]] == labels[(size_t)o.perm[(size_t)a]]) b++;
    for (int64_t p = a; p < b; p++) o.seg_end[(size_t)p] = (int32_t)b;
    o.largest = std::max(o.largest, b - a);
    a = b;
  }
  return o;
}

extern "C" int somhip_class_nearest_later(somhip_dataset *ds, float *min_sq, int32_t *state) try {
  CHK(check_dataset(ds, min_sq && state, "somhip_class_nearest_later"));
  if (ds->labels.empty()) return fail("somhip_class_nearest_later: the data set has no labels");
  const int64_t n = ds->n;
  if (n > 0x7FFFFFFFll - 2 * CLASS_CHUNK) return fail("somhip_class_nearest_later: %lld rows are more than this path indexes", (long long)n);
  somhip_engine *e = ds->e;
  HIPCHK(hipSetDevice(e->device));
  const int d = ds->d, d4 = (d + 3) / 4;
  const int64_t groups = (n + WAVE - 1) / WAVE, padded = groups * WAVE;
  const ClassOrder o = class_order(ds->labels, groups);
  const int64_t blocks = (n + CLASS_ROWS - 1) / CLASS_ROWS;
  // later positions a row of a block can need: up to the end of the class of the block's last row
  const int64_t chunks = (CLASS_ROWS - 1 + o.largest + CLASS_CHUNK - 1) / CLASS_CHUNK;
  if (chunks > 65535) return fail("somhip_class_nearest_later: a class of %lld rows is more than this path indexes", (long long)o.largest);
  const bool masked = ds->d_mask != nullptr;

  int32_t *d_perm, *d_end; float4 *d_tiles; uint32_t *d_mtiles = nullptr, *d_min, *d_flag;
  CHK(scratch(e, SLOT_CALL_A, (size_t)n, &d_perm));
  CHK(scratch(e, SLOT_CALL_B, (size_t)padded, &d_end));
  CHK(scratch(e, SLOT_STAGE, (size_t)padded * d4, &d_tiles));
  if (masked) CHK(scratch(e, SLOT_SAMPLES, (size_t)padded * d4, &d_mtiles));
  CHK(scratch(e, SLOT_PARTIAL, (size_t)padded, &d_min));
  CHK(scratch(e, SLOT_PAIRS, (size_t)padded, &d_flag));
  CHK(to_device(e, d_perm, o.perm.data(), (size_t)n));
  CHK(to_device(e, d_end, o.seg_end.data(), (size_t)padded));
  HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d_min, (int)CLASS_NONE_BITS, (size_t)padded, e->stream));
  HIPCHK(hipMemsetAsync(d_flag, 0, sizeof(uint32_t) * (size_t)padded, e->stream));
  if (masked)
    CHK(LAUNCH_TIMED(e, KID_LAYOUT, k_class_layout<true>, dim3((unsigned)groups), dim3(256), 0, ds->d_rows, ds->d_mask, d_perm, n, d, d4, d_tiles, d_mtiles));
  else
    CHK(LAUNCH_TIMED(e, KID_LAYOUT, k_class_layout<false>, dim3((unsigned)groups), dim3(256), 0, ds->d_rows, nullptr, d_perm, n, d, d4, d_tiles, nullptr));
  const dim3 grid((unsigned)blocks, (unsigned)chunks);
  if (masked)
    CHK(LAUNCH_TIMED(e, KID_CLASS_NEAREST, (k_class_nearest<CLASS_S_MASKED, true>), grid, dim3(256), 0, d_tiles, d_mtiles, d_end, n, d, d4, d_min, d_flag));
  else
    CHK(LAUNCH_TIMED(e, KID_CLASS_NEAREST, (k_class_nearest<CLASS_S, false>), grid, dim3(256), 0, d_tiles, nullptr, d_end, n, d, d4, d_min, d_flag));
  std::vector<uint32_t> hmin((size_t)n), hflag((size_t)n);
  CHK(to_host(e, hmin.data(), d_min, (size_t)n));
  CHK(to_host_sync(e, hflag.data(), d_flag, (size_t)n));
  for (int64_t p = 0; p < n; p++) {
    const int64_t r = o.perm[(size_t)p];
    memcpy(&min_sq[r], &hmin[(size_t)p], sizeof(float));
    state[r] = o.seg_end[(size_t)p] == p + 1 ? 0 : hflag[(size_t)p] ? 2 : 1;
  }
  return 0;
} ABI_CATCH(somhip_class_nearest_later)
