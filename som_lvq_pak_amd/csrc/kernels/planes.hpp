// kernels/planes.hpp -- grey-scaled component planes of a codebook (SOM_PAK planes.c:146-186), bit for bit
// (part of kernels.hpp; see the notes at the top of that file)
//
// For component c of every row, in the reference's row order k:
//   minval, maxval   over the rows, found with `if (maxval < p)` / `if (minval > p)` in row order, so of several rows that
//                    compare equal (+0.0 and -0.0) the first one's bits stay
//   cv               0.5 when the float difference maxval - minval is 0, else
//                    (float)(0.05 + 0.9 * (double)(float)(p - minval) / (double)(float)(maxval - minval)):
//                    two float subtractions, then a product, a quotient and a sum that each round in double
// The rows are read where they lie, as row-group tiles (64 rows x d4 float4 chunks): a wave takes one chunk of one row
// group, 64 float4 = 1 KiB, and has up to four planes of 64 rows in its registers.  Three kernels:
//
//   k_planes_minmax  per plane two 64-bit keys, both reduced with an unsigned minimum:
//                      lo key = (order(p) << 32) | unit      hi key = (~order(p) << 32) | unit
//                    order() maps float bits to unsigned integers of the same order (negative floats do not order as
//                    their bit patterns) with both zeros at one value, so the smallest key is the extreme value at the
//                    first unit that holds it -- the row whose bits the reference keeps.  The reference starts from
//                    minval = FLT_MAX and maxval = -FLT_MAX, so NaN wins no comparison and gets no key, a value
//                    >= FLT_MAX (+inf) gets no lo key and a value <= -FLT_MAX (-inf) no hi key: a column of +inf alone
//                    keeps minval = FLT_MAX.  Padding lanes of the last row group and padding dims of the last
//                    chunk get no key either.  Every wave walks a slab of row groups and leaves its keys in a table
//                    of partial results; no atomics (with one pair of words per plane, the 64 to 128 waves that meet
//                    at each word took as long as the read of the rows: profiles/planes_vs_host.txt).
//   k_planes_bounds  one wave per plane: the minimum over the slabs' keys, then the component at the key's unit (its
//                    bits, the sign of a zero included) into lo[] / hi[]; FLT_MAX / -FLT_MAX where no row had a key
//   k_planes_grey    cv of every (plane, row), plane-major: grey[j * n + unit]
//
// fp32 denormals are kept (the default for this target), fp64 division is the correctly rounded one and nothing is
// contracted at this library's build flags (see sammon.hpp).
#pragma once
#include "common.hpp"

namespace somhip {

// As umat.hpp: a translation unit of their own (csrc/planes.hip defines SOMHIP_PLANES_DEFINE), so the code object of the
// training kernels stays what it is without them.  somhip.hip sees the declarations.
// Both tile kernels: blockDim.x == 256, wave w of block b takes chunk q0 + (b % chunk_blocks) * 4 + w; k_planes_minmax
// walks the row groups of slab b / chunk_blocks: that one, + n_slabs, ...; k_planes_grey takes row group b / chunk_blocks
// alone.  part[2 * n_planes][n_slabs]: row 2j the lo keys, row 2j + 1 the hi keys of plane first + j, one per slab.
__global__ __launch_bounds__(256) void k_planes_minmax(CbView cb, int first, int n_planes, int chunk_blocks, int n_slabs,
                                                       unsigned long long *__restrict__ part);
__global__ __launch_bounds__(256) void k_planes_bounds(CbView cb, int first, int n_planes, int n_slabs,
                                                       const unsigned long long *__restrict__ part, float *__restrict__ lo,
                                                       float *__restrict__ hi);
__global__ __launch_bounds__(256) void k_planes_grey(CbView cb, int first, int n_planes, int chunk_blocks,
                                                     const float *__restrict__ lo, const float *__restrict__ hi,
                                                     float *__restrict__ grey);

#ifdef SOMHIP_PLANES_DEFINE

// float bits -> unsigned integers in the floats' order; -0.0 and +0.0 both give 0x80000000
__device__ __forceinline__ uint32_t planes_order(float v) {
  const uint32_t b = v == 0.0f ? 0u : __float_as_uint(v);
  return b ^ (static_cast<uint32_t>(static_cast<int32_t>(b) >> 31) | 0x80000000u);
}

// a lo key only for p < FLT_MAX and a hi key only for p > -FLT_MAX: the comparisons the reference's start values lose
__device__ __forceinline__ void planes_keys(float p, uint32_t unit, bool take, uint64_t &klo, uint64_t &khi) {
  if (!take) return;
  const uint32_t o = planes_order(p);
  const uint64_t a = (static_cast<uint64_t>(o) << 32) | unit, b = (static_cast<uint64_t>(~o) << 32) | unit;
  klo = (p < __uint_as_float(FLT_MAX_BITS) && a < klo) ? a : klo;
  khi = (p > -__uint_as_float(FLT_MAX_BITS) && b < khi) ? b : khi;
}

// =====================================================================================
// K-planes-minmax: a lane keeps its own eight keys over the row groups of its slab; one wave reduction, then every
// (plane of the window, slab) entry of `part` is written by exactly one wave, KEY_NONE where no row had a key.
// =====================================================================================
__global__ __launch_bounds__(256) void k_planes_minmax(CbView cb, int first, int n_planes, int chunk_blocks, int n_slabs,
                                                       unsigned long long *__restrict__ part) {
  const int lane = threadIdx.x & 63;
  const int q = (first >> 2) + static_cast<int>(blockIdx.x % static_cast<unsigned>(chunk_blocks)) * 4 + (threadIdx.x >> 6);
  if (q >= cb.d4 || q * 4 >= first + n_planes) return;           // wave-uniform; no barrier follows
  const int slab = static_cast<int>(blockIdx.x / static_cast<unsigned>(chunk_blocks));
  if (slab >= n_slabs) return;
  bool in[4];
#pragma unroll
  for (int j = 0; j < 4; j++) in[j] = q * 4 + j >= first && q * 4 + j < first + n_planes;     // < d: the host checked the window
  uint64_t klo[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE}, khi[4] = {KEY_NONE, KEY_NONE, KEY_NONE, KEY_NONE};
  for (int64_t g = slab; g < cb.ngroups; g += n_slabs) {
    const int64_t row = g * WAVE + lane;
    const bool live = row < cb.n;
    const float4 v = *tile_ptr(cb, g, q, lane);                   // padding rows are allocated (and zero)
    const uint32_t unit = live ? unit_of_row(cb, row) : 0u;
    planes_keys(v.x, unit, live && in[0], klo[0], khi[0]);
    planes_keys(v.y, unit, live && in[1], klo[1], khi[1]);
    planes_keys(v.z, unit, live && in[2], klo[2], khi[2]);
    planes_keys(v.w, unit, live && in[3], klo[3], khi[3]);
  }
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (!in[j]) continue;
    const uint64_t a = wave_min_u64(klo[j]), b = wave_min_u64(khi[j]);
    if (lane == 0) {
      const int64_t p = q * 4 + j - first;
      part[(2 * p) * n_slabs + slab] = a;
      part[(2 * p + 1) * n_slabs + slab] = b;
    }
  }
}

// K-planes-bounds: wave w of block b takes plane 4 b + w: the smallest key of each of its two rows of `part`, then the
// component at that key's unit.  The codebook is a whole one (row_offset 0, no interleave).  blockDim.x == 256.
__global__ __launch_bounds__(256) void k_planes_bounds(CbView cb, int first, int n_planes, int n_slabs,
                                                       const unsigned long long *__restrict__ part, float *__restrict__ lo,
                                                       float *__restrict__ hi) {
  const int lane = threadIdx.x & 63;
  const int p = static_cast<int>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (p >= n_planes) return;                                      // wave-uniform
  const int c = first + p;
  float out[2] = {__uint_as_float(FLT_MAX_BITS), __uint_as_float(FLT_MAX_BITS | 0x80000000u)};
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const unsigned long long *keys = part + (2 * static_cast<int64_t>(p) + s) * n_slabs;
    uint64_t key = KEY_NONE;
    for (int k = lane; k < n_slabs; k += WAVE) key = keys[k] < key ? keys[k] : key;
    key = wave_min_u64(key);
    if (key == KEY_NONE || static_cast<int64_t>(static_cast<uint32_t>(key)) >= cb.n) continue;
    const int64_t row = row_of_unit(cb, static_cast<uint32_t>(key));
    out[s] = reinterpret_cast<const float *>(tile_ptr(cb, row >> 6, c >> 2, static_cast<int>(row & 63)))[c & 3];
  }
  if (lane == 0) {
    lo[p] = out[0];
    hi[p] = out[1];
  }
}

// (float)(0.05 + 0.9 * (p - minval) / (maxval - minval)) under C's promotions, planes.c:172-176
__device__ __forceinline__ float planes_cv(float p, float minval, float range) {
  if (range == 0.0f) return 0.5f;
  const float num = p - minval;
  const double prod = 0.9 * static_cast<double>(num);
  const double quot = prod / static_cast<double>(range);
  return static_cast<float>(0.05 + quot);
}

// =====================================================================================
// K-planes-grey: one wave = one chunk of one row group; up to four plane segments of 64 floats go out.  In the
// reference's row order a segment is 256 contiguous bytes; in 8x8 patch order it is eight runs of 32 bytes.
// =====================================================================================
__global__ __launch_bounds__(256) void k_planes_grey(CbView cb, int first, int n_planes, int chunk_blocks,
                                                     const float *__restrict__ lo, const float *__restrict__ hi,
                                                     float *__restrict__ grey) {
  const int lane = threadIdx.x & 63;
  const int q = (first >> 2) + static_cast<int>(blockIdx.x % static_cast<unsigned>(chunk_blocks)) * 4 + (threadIdx.x >> 6);
  if (q >= cb.d4 || q * 4 >= first + n_planes) return;
  const int64_t g = blockIdx.x / static_cast<unsigned>(chunk_blocks);
  const int64_t row = g * WAVE + lane;
  if (g >= cb.ngroups || row >= cb.n) return;
  const float4 v = *tile_ptr(cb, g, q, lane);
  const float comp[4] = {v.x, v.y, v.z, v.w};
  const int64_t unit = unit_of_row(cb, row);
  if (unit >= cb.n) return;                                       // a whole codebook: never
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int p = q * 4 + j - first;
    if (p < 0 || p >= n_planes) continue;
    const float minval = lo[p], maxval = hi[p];
    grey[static_cast<int64_t>(p) * cb.n + unit] = planes_cv(comp[j], minval, maxval - minval);
  }
}

#endif  // SOMHIP_PLANES_DEFINE

}  // namespace somhip
