// host_planes.inc -- grey-scaled component planes of a codebook (kernels/planes.hpp)
// (part of somhip.hip: same translation unit)
//
// The kernel id table is closed (its length and last entries are part of what callers rely on), so these three launches
// carry no LaunchTimer; tools/planes_measure.py times them from a kernel trace.

extern "C" int somhip_planes(somhip_codebook *cb, int first_plane, int n_planes, float *grey, float *lo, float *hi) try {
  CHK(check_codebook(cb, grey, "somhip_planes"));
  if (is_shard(cb))
    return fail("somhip_planes: the codebook is a shard (%lld of %lld rows); the planes need every row",
                (long long)cb->v.n, (long long)cb->n_global);
  if (n_planes < 1) return fail("somhip_planes: %d planes asked for (at least 1)", n_planes);
  if (first_plane < 0 || first_plane >= cb->v.d || n_planes > cb->v.d - first_plane)
    return fail("somhip_planes: planes %d to %lld are outside the codebook's %d components", first_plane,
                (long long)first_plane + n_planes - 1, cb->v.d);
  if (cb->v.n < 1 || cb->v.n > 0xFFFFFFFFll) return fail("somhip_planes: %lld rows are more than this path indexes", (long long)cb->v.n);
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  const int64_t n = cb->v.n;
  const size_t total = (size_t)n_planes * (size_t)n;
  const int q0 = first_plane >> 2, nq = ((first_plane + n_planes - 1) >> 2) - q0 + 1;
  const int chunk_blocks = (nq + 3) / 4;
  // enough waves to fill the device; each walks the row groups of one slab with its keys in registers and leaves them
  // in its own column of the table of partial keys
  const int64_t want = std::max<int64_t>(1, (int64_t)(e->n_cus > 0 ? e->n_cus : 256) * 8 / chunk_blocks);
  const int n_slabs = (int)std::min<int64_t>(cb->v.ngroups, want);
  float *d_grey, *d_lo; unsigned long long *d_part;
  CHK(scratch(e, SLOT_CALL_A, total, &d_grey));
  CHK(scratch(e, SLOT_PARTIAL, 2 * (size_t)n_planes * (size_t)n_slabs, &d_part));
  CHK(scratch(e, SLOT_CALL_B, 2 * (size_t)n_planes, &d_lo));      // the planes' lo, then their hi
  float *d_hi = d_lo + n_planes;
  const int64_t grey_blocks = (int64_t)chunk_blocks * cb->v.ngroups;
  if (grey_blocks > 0x7FFFFFFFll) return fail("somhip_planes: %lld workgroups are more than one launch takes", (long long)grey_blocks);
  CHK(LAUNCH(e, k_planes_minmax, dim3((unsigned)(chunk_blocks * n_slabs)), dim3(256), 0, cb->v, first_plane, n_planes, chunk_blocks, n_slabs,
      d_part));
  CHK(LAUNCH(e, k_planes_bounds, dim3((unsigned)((n_planes + 3) / 4)), dim3(256), 0, cb->v, first_plane, n_planes, n_slabs, d_part, d_lo, d_hi));
  CHK(LAUNCH(e, k_planes_grey, dim3((unsigned)grey_blocks), dim3(256), 0, cb->v, first_plane, n_planes, chunk_blocks, d_lo, d_hi, d_grey));
  if (lo) CHK(to_host(e, lo, d_lo, (size_t)n_planes));
  if (hi) CHK(to_host(e, hi, d_hi, (size_t)n_planes));
  return to_host_sync(e, grey, d_grey, total);
} ABI_CATCH(somhip_planes)
