// host_umat.inc -- the U-matrix of a map codebook (kernels/umat.hpp)
// (part of somhip.hip: same translation unit)

extern "C" int somhip_umatrix(somhip_codebook *cb, int filters, float *u, double minmax[2]) try {
  CHK(check_codebook(cb, u, "somhip_umatrix"));
  if (cb->v.topol != SOMHIP_TOPOL_HEXA && cb->v.topol != SOMHIP_TOPOL_RECT)
    return fail("somhip_umatrix: the codebook is not a map (topology %d): only hexa and rect maps have a U-matrix", cb->v.topol);
  if (is_shard(cb))
    return fail("somhip_umatrix: the codebook is a shard (%lld of %lld rows); the U-matrix needs the whole map",
                (long long)cb->v.n, (long long)cb->n_global);
  const int mx = cb->v.xdim, my = cb->ydim;
  if ((int64_t)mx * my != cb->v.n) return fail("somhip_umatrix: a %d x %d map does not have %lld rows", mx, my, (long long)cb->v.n);
  if (mx < 2 || my < 2) return fail("somhip_umatrix: a %d x %d map has no U-matrix (both sides must be at least 2)", mx, my);
  if (mx > 16384 || my > 16384) return fail("somhip_umatrix: a %d x %d map is more than this path indexes", mx, my);
  if (filters & ~(SOMHIP_UMAT_AVERAGE | SOMHIP_UMAT_MEDIAN)) return fail("somhip_umatrix: unknown filter bits 0x%x", filters);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  UmatDims m;
  m.mx = mx; m.my = my; m.ux = 2 * mx - 1; m.uy = 2 * my - 1; m.topol = cb->v.topol;
  const int64_t count = (int64_t)m.ux * m.uy;
  float *cur, *other; uint32_t *d_mm;
  CHK(scratch(e, SLOT_CALL_A, (size_t)count, &cur));
  CHK(scratch(e, SLOT_CALL_B, (size_t)count, &other));
  CHK(scratch(e, SLOT_PARTIAL, 2, &d_mm));
  const uint32_t preset[2] = {FLT_MAX_BITS, 0u};
  CHK(to_device(e, d_mm, preset, 2));
  const unsigned per_entry = (unsigned)((count + 255) / 256);
  CHK(LAUNCH_TIMED(e, KID_UMAT_DIST, k_umat_dist, dim3((unsigned)((cb->v.n + 255) / 256), 3), dim3(256), 0, cb->v, m, cur));
  CHK(LAUNCH_TIMED(e, KID_UMAT_UNITS, k_umat_units, dim3((unsigned)((cb->v.n + 255) / 256)), dim3(256), 0, m, cur));
  CHK(LAUNCH_TIMED(e, KID_UMAT_MINMAX, k_umat_minmax, dim3(std::min(per_entry, 128u)), dim3(256), 0, cur, count, d_mm));
  uint32_t bits[2];
  CHK(to_host_sync(e, bits, d_mm, 2));
  float fmin, fmax;
  memcpy(&fmin, &bits[0], sizeof fmin);
  memcpy(&fmax, &bits[1], sizeof fmax);
  const double lo = (double)fmin, hi = (double)fmax;
  if (minmax) { minmax[0] = lo; minmax[1] = hi; }
  if (hi == lo)
    return fail("somhip_umatrix: every distance between neighbouring units is %g: the scaling to [0, 1] would divide by zero", lo);
  CHK(LAUNCH_TIMED(e, KID_UMAT_SCALE, k_umat_scale, dim3(per_entry), dim3(256), 0, cur, count, lo, hi - lo));
  if (filters & SOMHIP_UMAT_AVERAGE) {
    CHK(LAUNCH_TIMED(e, KID_UMAT_AVERAGE, k_umat_average, dim3(per_entry), dim3(256), 0, m, cur, other));
    std::swap(cur, other);
  }
  if (filters & SOMHIP_UMAT_MEDIAN) {
    CHK(LAUNCH_TIMED(e, KID_UMAT_MEDIAN, k_umat_median, dim3(per_entry), dim3(256), 0, m, cur, other));
    std::swap(cur, other);
  }
  return to_host_sync(e, u, cur, (size_t)count);
} ABI_CATCH(somhip_umatrix)
