// kernels/ngas.hpp -- K10: batch neural gas -- the rank entries behind the k-NN search, the per-unit ordered fp64 sums of
// rank-weighted data rows, and the update
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "glvq.hpp"

namespace somhip {

// =====================================================================================
// K10: one epoch of batch neural gas (the definition is in include/somhip.h).  Behind the exact
// k-NN search of every sample against the frozen codebook (find_winner_knn's order of equal distances), the data in
// segments of a bounded number of (sample, rank) pairs:
//
//   entries  k_ng_entries, per search chunk: the pair (unit, sample in segment << 8 | rank) of every sample and every rank
//            r < K at position sample * K + r, the segment's counts by integer atomics, the rank-0 distance for the q chain.
//   group    K8's k_batchmap_starts and the stable sort of the pairs by unit (the host, rocPRIM): list[starts[u] ..
//            starts[u + 1]) holds the packed values of unit u in data order -- a sample ranks a unit at most once.
//   sums     k_ng_sums: [S | W][u][k] = one chain of fp64 additions over the unit's list of w[rank] * (double)x[k] -- a
//            multiply, then an add -- with w from the epoch's table.  k_ng_sums<true> continues the chains the segments
//            before this one left, so the cut into segments does not show in the bits.
//   update   k_ng_update: m_j[k] = (float)(S[j][k] / W[j]) over the storage tiles, in place, where W[j] > 0.
//
// No floating-point atomics anywhere: every sum is a function of the data, the codebook and the schedule alone.
// =====================================================================================
constexpr int NG_THREADS = 256;               // the entries pass and the update
constexpr int NG_RANK_BITS = 8;               // a packed list value: sample in segment << 8 | rank (rank < SOMHIP_KNN_MAX = 256)
constexpr int NG_SUM_AHEAD = 16;              // list entries requested ahead of the chain (measured at 4, 8, 16: profiles/ngas_epoch.txt)
static_assert(KNN_WIDE_MAX <= (1 << NG_RANK_BITS), "a rank fits the low bits of a packed list value");

// Per (sample s of the chunk, rank r < K) from keys[s][stride] (ascending; inverted: tags are ~unit, find_winner_knn's
// order): at position (off + s) * K + r of the segment's arrays, unit = the r-th nearest unit and packed = (off + s) << 8 | r;
// a slot without a row (KEY_NONE, or nothing below FLT_MAX) gets unit = n_units, which sorts behind every list.
// hits[unit]++ for a live slot.  d0 (null: not wanted) [s] = the rank-0 squared distance, -1 without one.  off: the chunk's
// first sample in the segment; (off + count) <= 2^24.
__global__ __launch_bounds__(NG_THREADS) void k_ng_entries(const uint64_t *__restrict__ keys, int stride, int K, int inverted,
                                                           int64_t off, int64_t count, uint32_t n_units,
                                                           uint32_t *__restrict__ unit, uint32_t *__restrict__ packed,
                                                           float *__restrict__ d0, uint32_t *__restrict__ hits) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * NG_THREADS + threadIdx.x;
  if (t >= count * K) return;
  const int64_t smp = t / K;
  const int r = static_cast<int>(t - smp * K);
  const uint64_t k = keys[smp * stride + r];
  const uint32_t bits = static_cast<uint32_t>(k >> 32), tag = static_cast<uint32_t>(k);
  const uint32_t u = inverted ? ~tag : tag;
  const bool live = bits < FLT_MAX_BITS && u < n_units;
  const int64_t pos = (off + smp) * K + r;
  unit[pos] = live ? u : n_units;
  packed[pos] = (static_cast<uint32_t>(off + smp) << NG_RANK_BITS) | static_cast<uint32_t>(r);
  if (live) atomicAdd(hits + u, 1u);
  if (d0 && r == 0) d0[smp] = live ? __uint_as_float(bits) : -1.0f;
}

// One wave per (unit u = blockIdx.x, 64 columns of [S | W]), lane = column k.  S[u][k], k < d: the chain of fp64 additions
// of w[r] * (double)x_s[k] -- a multiply, then an add -- over the unit's list in data order, where a list value is
// s << 8 | r, sample s of the segment is data row (first + s) % n_rows (first, s < n_rows) and w is the epoch's table of K
// doubles; column k = d: the same chain over w[r] alone (w * 1.0 is w).  S is [n_units][d + 1]; total[u] is the length of
// the unit's lists.  The list is known, so NG_SUM_AHEAD entries -- the packed value, its weight (both at wave-uniform
// addresses), the row element -- are requested before their additions run.
// CONT: the data come in segments and S, total hold what the segments before this one left: the chain goes on from
// S[u][k], the count grows.  A chain from a stored value is the same chain, so the segments leave the bits of one
// segment over all the samples.  An instantiation of its own: the first segment starts from +0.0 with no load of S.
template <bool CONT>
__global__ __launch_bounds__(BM_SUM_DIMS) void k_ng_sums(const float *__restrict__ rows, int64_t n_rows, int d, int64_t first,
                                                         const uint32_t *__restrict__ list, const uint32_t *__restrict__ starts,
                                                         const double *__restrict__ w, double *__restrict__ S,
                                                         uint32_t *__restrict__ total) {
  const uint32_t u = blockIdx.x;
  const int k = static_cast<int>(blockIdx.y) * BM_SUM_DIMS + static_cast<int>(threadIdx.x);
  const uint32_t lo = starts[u], hi = starts[u + 1];
  if (k > d) return;
  if (k == d) total[u] = CONT ? total[u] + (hi - lo) : hi - lo;
  double *out = S + static_cast<int64_t>(u) * (d + 1) + k;
  if (lo == hi) {                                             // no sample of this segment: the chain stands, or starts and ends at +0.0
    if (!CONT) *out = 0.0;
    return;
  }
  // No branch between an entry and its row element, so that the loads of the entries ahead are all in flight at once: the
  // row wraps by one select (a segment is no longer than the data set: first + s < 2 n_rows), and the lane of column d
  // loads column d - 1 and drops it.
  const int kc = min(k, d - 1);
  auto elem = [&](uint32_t v) -> float {
    int64_t r = first + static_cast<int64_t>(v >> NG_RANK_BITS);
    r -= r >= n_rows ? n_rows : 0;
    const float x = rows[r * d + kc];
    return k < d ? x : 1.0f;
  };
  constexpr uint32_t RANK = (1u << NG_RANK_BITS) - 1;
  double acc = CONT ? *out : 0.0;
  uint32_t i = lo;
  // Three dependent requests stand before an addition: the packed value, then its weight and its row element.  Each kind
  // is asked for NG_SUM_AHEAD entries at a time, in loops of their own so that the requests leave back to back, and the
  // packed values of the next batch (clamped to the list, so without a branch) while this batch's rows are on their way.
  uint32_t v[NG_SUM_AHEAD];
#pragma unroll
  for (int a = 0; a < NG_SUM_AHEAD; a++) v[a] = list[min(i + a, hi - 1)];
  for (; hi - i >= NG_SUM_AHEAD; i += NG_SUM_AHEAD) {
    float x[NG_SUM_AHEAD];
    double wt[NG_SUM_AHEAD];
#pragma unroll
    for (int a = 0; a < NG_SUM_AHEAD; a++) wt[a] = w[v[a] & RANK];
#pragma unroll
    for (int a = 0; a < NG_SUM_AHEAD; a++) x[a] = elem(v[a]);
#pragma unroll
    for (int a = 0; a < NG_SUM_AHEAD; a++) v[a] = list[min(i + NG_SUM_AHEAD + a, hi - 1)];
#pragma unroll
    for (int a = 0; a < NG_SUM_AHEAD; a++) {
      const double p = wt[a] * static_cast<double>(x[a]);
      acc += p;
    }
  }
  for (; i < hi; i++) {
    const uint32_t v = list[i];
    const double p = w[v & RANK] * static_cast<double>(elem(v));
    acc += p;
  }
  *out = acc;
}

// In place over the storage tiles: thread = (row group, chunk of 4 dims, lane).  m_j[k] = (float)(S[j][k] / W[j]) with
// W[j] = S[j][d]: one fp64 division, one rounding to float.  A row with W == 0 -- outside every sample's first K ranks,
// or with weights that all underflowed -- keeps its bits; so does the padding.
__global__ __launch_bounds__(NG_THREADS) void k_ng_update(CbView cb, const double *__restrict__ S) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * NG_THREADS + threadIdx.x;
  const int lane = static_cast<int>(t & (WAVE - 1));
  const int64_t gq = t >> 6;
  if (gq >= cb.ngroups * cb.d4) return;
  const int64_t g = gq / cb.d4;
  const int q = static_cast<int>(gq % cb.d4);
  const int64_t row = g * WAVE + lane;
  if (row >= cb.n) return;
  const double *Su = S + static_cast<int64_t>(unit_of_row(cb, row)) * (cb.d + 1);
  const double W = Su[cb.d];
  if (!(W > 0.0)) return;
  float4 *cp = tile_ptr_w(cb, g, q, lane);
  const float4 c = *cp;
  float v[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int k = q * 4 + j;
    if (k < cb.d) v[j] = static_cast<float>(Su[k] / W);
  }
  *cp = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace somhip
