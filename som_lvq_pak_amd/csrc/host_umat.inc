// host_umat.inc -- the U-matrix of a map codebook (kernels/umat.hpp)
// (part of somhip.hip: same translation unit)

extern "C" int somhip_umatrix(somhip_codebook *cb, int filters, float *u, double minmax[2]) try {
  if (!cb || !u) return fail("somhip_umatrix: null argument");
  if (!cb->e) return fail("somhip_umatrix: the engine of this codebook was destroyed");
  if (cb->v.topol != SOMHIP_TOPOL_HEXA && cb->v.topol != SOMHIP_TOPOL_RECT)
    return fail("somhip_umatrix: the codebook is not a map (topology %d): only hexa and rect maps have a U-matrix", cb->v.topol);
  if (cb->v.patch_stride > 1 || cb->v.row_offset != 0 || cb->v.n != cb->n_global)
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
  HIPCHK(hipMemcpyAsync(d_mm, preset, sizeof preset, hipMemcpyHostToDevice, e->stream));
  const unsigned per_entry = (unsigned)((count + 255) / 256);
  {
    LaunchTimer t(e, KID_UMAT_DIST);
    hipLaunchKernelGGL(k_umat_dist, dim3((unsigned)((cb->v.n + 255) / 256), 3), dim3(256), 0, e->stream, cb->v, m, cur);
  }
  HIPCHK(hipGetLastError());
  {
    LaunchTimer t(e, KID_UMAT_UNITS);
    hipLaunchKernelGGL(k_umat_units, dim3((unsigned)((cb->v.n + 255) / 256)), dim3(256), 0, e->stream, m, cur);
  }
  HIPCHK(hipGetLastError());
  {
    LaunchTimer t(e, KID_UMAT_MINMAX);
    hipLaunchKernelGGL(k_umat_minmax, dim3(std::min(per_entry, 128u)), dim3(256), 0, e->stream, (const float *)cur, count, d_mm);
  }
  HIPCHK(hipGetLastError());
  uint32_t bits[2];
  HIPCHK(hipMemcpyAsync(bits, d_mm, sizeof bits, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  float fmin, fmax;
  memcpy(&fmin, &bits[0], sizeof fmin);
  memcpy(&fmax, &bits[1], sizeof fmax);
  const double lo = (double)fmin, hi = (double)fmax;
  if (minmax) { minmax[0] = lo; minmax[1] = hi; }
  if (hi == lo)
    return fail("somhip_umatrix: every distance between neighbouring units is %g: the scaling to [0, 1] would divide by zero", lo);
  {
    LaunchTimer t(e, KID_UMAT_SCALE);
    hipLaunchKernelGGL(k_umat_scale, dim3(per_entry), dim3(256), 0, e->stream, cur, count, lo, hi - lo);
  }
  HIPCHK(hipGetLastError());
  if (filters & SOMHIP_UMAT_AVERAGE) {
    {
      LaunchTimer t(e, KID_UMAT_AVERAGE);
      hipLaunchKernelGGL(k_umat_average, dim3(per_entry), dim3(256), 0, e->stream, m, (const float *)cur, other);
    }
    HIPCHK(hipGetLastError());
    std::swap(cur, other);
  }
  if (filters & SOMHIP_UMAT_MEDIAN) {
    {
      LaunchTimer t(e, KID_UMAT_MEDIAN);
      hipLaunchKernelGGL(k_umat_median, dim3(per_entry), dim3(256), 0, e->stream, m, (const float *)cur, other);
    }
    HIPCHK(hipGetLastError());
    std::swap(cur, other);
  }
  HIPCHK(hipMemcpyAsync(u, cur, sizeof(float) * (size_t)count, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_umatrix)
