// kernels/class_nearest.hpp -- K-class: within-class nearest LATER row of a data set, exact
// (part of kernels.hpp; see the notes at the top of that file)
//
// med_distances / min_distances (lvq_rout.c:280-491): for every entry, the smallest vector_dist_euc
// (lvq_pak.c:291-316) to a later entry of the same class.  The distance is the fp32 sum of (a_i - b_i)^2 in the
// order of i, three roundings per component; a component masked in EITHER row is skipped; (float) sqrt((double) sum)
// is monotone, so the minimum is taken over the sums and the host takes the root.
//
// The host orders the rows by class with a stable permutation, so a class is one contiguous segment of positions
// and "later row of the same class" is "higher position below the segment's end".  The rows are stored once, in
// that order, as row-group tiles (kernels.hpp): T[g][q][lane], position = 64 g + lane.  The same array serves as
// the sample tiles of scan_exact.hpp: the S float4 of positions [ts, ts + S) at chunk q are contiguous when S
// divides 64 and ts is a multiple of S.
#pragma once
#include "sammon.hpp"

namespace somhip {

constexpr int CLASS_ROWS = 256;      // positions per workgroup (4 waves, one lane = one row)
constexpr int CLASS_CHUNK = 256;     // later positions one workgroup compares them with
constexpr uint32_t CLASS_NONE_BITS = 0x7F800000u;   // +inf: no later row at a finite distance (yet)

// =====================================================================================
// K-class-layout: rows[perm[pos]] -> T[g][q][lane] (zero rows from n on, zero components from d on) and, MASKED,
// the mask of the same four components as the low bits of MT[g][q][lane].  grid = row groups.
// =====================================================================================
template <bool MASKED>
__global__ __launch_bounds__(256) void k_class_layout(const float *__restrict__ rows, const uint8_t *__restrict__ mask,
                                                      const int32_t *__restrict__ perm, int64_t n, int d, int d4,
                                                      float4 *__restrict__ T, uint32_t *__restrict__ MT) {
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int64_t pos = g * WAVE + lane;
  const int64_t src = pos < n ? static_cast<int64_t>(perm[pos]) : -1;
  for (int q = threadIdx.x >> 6; q < d4; q += blockDim.x >> 6) {
    float v[4];
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int i = q * 4 + j;
      const bool in = src >= 0 && i < d;
      v[j] = in ? rows[src * d + i] : 0.0f;
      if (MASKED && in && mask[src * d + i] != 0) bits |= 1u << j;
    }
    const int64_t at = (g * d4 + q) * WAVE + lane;
    T[at] = make_float4(v[0], v[1], v[2], v[3]);
    if (MASKED) MT[at] = bits;
  }
}

// =====================================================================================
// K-class: one lane = one row (position pr), S later positions of a tile as running sums in registers, their values
// read at wave-uniform addresses, as in K1 (scan_exact.hpp).  A pair (pr, ps) counts when pr < ps < seg_end[pr].
//
// grid.x = blocks of 256 positions, grid.y = chunks of 256 later positions counted from the block's first position:
// the host sizes grid.y by the largest class, so the grid holds no pair of positions further apart than a class can
// be.  A workgroup whose chunk starts at or past the segment end of its last row returns at once (about half of
// the chunks of a large class: the triangle); a wave skips the tiles that lie before its first row or past the
// segment end of its last one.
//
// seg_end[pos] (int32, padded with 0 to whole row groups) = end of the class segment that holds pos.
// min_bits[pos], preset to CLASS_NONE_BITS: bit pattern of the smallest finite sum (sums are >= +0, so their bit
// patterns order as unsigned integers; an infinite or NaN sum never passes `dist < FLT_MAX` in the reference and
// never beats the preset here).  MASKED: every skipped component is counted; a counted pair with all d components
// skipped (vector_dist_euc returns -1) sets all_masked[pos].
// Padding components (i >= d) are 0 - 0: adding their +0.0 square to a sum that is >= +0.0 is exact.
// =====================================================================================
template <int S, bool MASKED>
__global__ __launch_bounds__(256) void k_class_nearest(const float4 *__restrict__ T, const uint32_t *__restrict__ MT,
                                                       const int32_t *__restrict__ seg_end, int64_t n, int d, int d4,
                                                       uint32_t *__restrict__ min_bits,
                                                       uint32_t *__restrict__ all_masked) {
  static_assert(WAVE % S == 0 && CLASS_CHUNK % S == 0 && CLASS_ROWS == 4 * WAVE, "tiles of S positions inside a row group");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * CLASS_ROWS;
  const int64_t cs = r0 + static_cast<int64_t>(blockIdx.y) * CLASS_CHUNK;
  if (cs >= n) return;
  const int64_t r_last = r0 + CLASS_ROWS - 1 < n ? r0 + CLASS_ROWS - 1 : n - 1;
  if (cs >= seg_end[r_last]) return;
  const int64_t w0 = r0 + static_cast<int64_t>(wave) * WAVE;
  if (w0 >= n) return;
  const int64_t w_last = w0 + WAVE - 1 < n ? w0 + WAVE - 1 : n - 1;
  const int64_t w_end = seg_end[w_last];                      // wave-uniform
  const int64_t pr = w0 + lane;
  const int64_t end_r = seg_end[pr];                          // 0 in the padding: no pair counts
  const int64_t g = w0 >> 6;
  const float4 *mine = T + g * d4 * WAVE + lane;
  const uint32_t *mine_m = MASKED ? MT + g * d4 * WAVE + lane : nullptr;

  uint32_t best = CLASS_NONE_BITS;
  bool none_shared = false;
  for (int t = 0; t < CLASS_CHUNK / S; t++) {
    const int64_t ts = cs + static_cast<int64_t>(t) * S;
    if (ts >= w_end) break;                                   // (w_end <= n: the tile below lies inside T)
    if (ts + S - 1 <= w0) continue;                           // nothing in it is later than this wave's first row
    const int64_t base = (ts >> 6) * d4 * WAVE + (ts & 63);
    const float4 *xs = T + base;
    const uint32_t *ms = MASKED ? MT + base : nullptr;
    float acc[S];
    int skipped[MASKED ? S : 1];
#pragma unroll
    for (int s = 0; s < S; s++) {
      acc[s] = 0.0f;
      if (MASKED) skipped[s] = 0;
    }
    for (int q = 0; q < d4; q++) {
      const float4 c = mine[static_cast<int64_t>(q) * WAVE];
      uint32_t cm = 0;
      if (MASKED) cm = mine_m[static_cast<int64_t>(q) * WAVE];
#pragma unroll
      for (int s = 0; s < S; s++) {
        const float4 x = xs[static_cast<int64_t>(q) * WAVE + s];           // wave-uniform address
        float a = acc[s];
        if (MASKED) {
          const uint32_t m = cm | ms[static_cast<int64_t>(q) * WAVE + s];  // either row's mask skips the component
          const float ax = sq_acc(a, c.x, x.x);
          a = (m & 1u) ? a : ax;
          const float ay = sq_acc(a, c.y, x.y);
          a = (m & 2u) ? a : ay;
          const float az = sq_acc(a, c.z, x.z);
          a = (m & 4u) ? a : az;
          const float aw = sq_acc(a, c.w, x.w);
          a = (m & 8u) ? a : aw;
          skipped[s] += __popc(m);
        } else {
          a = sq_acc(a, c.x, x.x);
          a = sq_acc(a, c.y, x.y);
          a = sq_acc(a, c.z, x.z);
          a = sq_acc(a, c.w, x.w);
        }
        acc[s] = a;
      }
    }
#pragma unroll
    for (int s = 0; s < S; s++) {
      const int64_t ps = ts + s;
      const bool counts = ps > pr && ps < end_r;
      const uint32_t bits = __float_as_uint(acc[s]);
      best = (counts && bits < best) ? bits : best;
      if (MASKED) none_shared = none_shared || (counts && skipped[s] == d);
    }
  }
  if (best != CLASS_NONE_BITS) atomicMin(min_bits + pr, best);
  if (MASKED && none_shared) atomicOr(all_masked + pr, 1u);
}

}  // namespace somhip
