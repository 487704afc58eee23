// kernels/ngas_dense.hpp -- K10d: dense batch neural gas -- the full ranking of every unit for every sample, turned into the
// weight matrix that K13's fp64 MFMA product sums
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "rslvq.hpp"

namespace somhip {

// =====================================================================================
// K10d: one epoch of dense batch neural gas (the definition is in include/somhip_ng_dense.h).  Per
// chunk of samples:
//
//   distances  K1w's k_knn_dist over k_pack_samples tiles, unchanged: dist[s][storage row], the exact fp32 sum of every row.
//   weights    k_ng_dense_weights: one workgroup per sample sorts the keys (distance bits, ~unit) of all its rows in LDS --
//              find_winner_knn's order, the later row first among equal distances -- and scatters Q[s][unit] = table[rank]
//              from the epoch's weight table (host arithmetic: no exp on the device).
//   sums       K13's k_rslvq_sums as it stands: [S | W] = Q^T x [X | 1] on v_mfma_f64_16x16x4_f64, continued over the chunks.
//   update     K10's k_ng_update: m_j[k] = (float)(S[j][k] / W[j]) where W[j] > 0.
//
// No floating-point arithmetic in this file at all: the kernel compares integers and copies doubles.
// =====================================================================================
constexpr int NGD_THREADS = 256;              // threads of a sample's workgroup
constexpr int NGD_MAX = 4096;                 // most rows of a codebook (include/somhip_ng_dense.h: SOMHIP_NG_DENSE_MAX): 32 KB of keys
static_assert((NGD_MAX & (NGD_MAX - 1)) == 0 && NGD_MAX * sizeof(uint64_t) <= 32768, "a sample's keys: 32 KB of LDS at most");

// Chunk sample i = blockIdx.x (< the grid), run sample off + i; dist[i][ld]: k_knn_dist's output, indexed by storage row.
// P: the smallest power of two >= cb.n (<= NGD_MAX); the launch gives P * 8 bytes of dynamic LDS.
//   keys      slot r < cb.n: (bits of dist[i][r]) << 32 | ~unit_of_row(r) -- distances are sums of squares, so their bits
//             order as the floats do; slots [cb.n, P): KEY_NONE, which sorts last
//   sort      the ascending bitonic network over P slots: per step thread t takes the pairs t, t + 256, ... of P / 2.
//             The two loads of a pair are ds_read_b64 at consecutive slots for the 32 lanes of a half wave while the
//             step's distance j >= 32 (one 256-B bank row: conflict-free) and at a stride of two slots in runs of j below
//             (lanes l and l + 16 of a half share a bank: 2-way); a pair is stored only where it was out of order
//   scatter   slot r < cb.n holds the unit of rank r: Q[i][unit] = table[r] where the distance is below FLT_MAX, else +0.0
//             (such rows sort behind the others by their bits); Q[i][cb.n .. ld) = +0.0, what k_rslvq_sums multiplies the
//             padding rows by.  table: the epoch's `cb.n` doubles, read by the lane whose slot is the rank -- consecutive
//             lanes, consecutive doubles.
// d0 (null: not wanted) [off + i] = the rank-0 squared distance, -1 where no row is below FLT_MAX.  rank_out, dunit_out
// (null: not wanted) [i][ld]: per unit its rank and its squared distance, for the tests.  Q may be null beside them.
__global__ __launch_bounds__(NGD_THREADS) void k_ng_dense_weights(CbView cb, const float *__restrict__ dist, int64_t ld, int64_t off, int P,
                                                                  const double *__restrict__ table, double *__restrict__ Q,
                                                                  float *__restrict__ d0, int32_t *__restrict__ rank_out,
                                                                  float *__restrict__ dunit_out) {
  extern __shared__ uint64_t ngd_keys[];
  const int tid = threadIdx.x;
  const int n = static_cast<int>(cb.n);
  const int64_t i = blockIdx.x;
  const float *drow = dist + i * ld;
  for (int r = tid; r < P; r += NGD_THREADS) ngd_keys[r] = r < n ? make_key(drow[r], ~unit_of_row(cb, r)) : KEY_NONE;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += NGD_THREADS) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // the pair's element with bit j clear
        const int hi = lo | j;
        const uint64_t a = ngd_keys[lo], b = ngd_keys[hi];
        if ((a > b) == ((lo & k) == 0)) { ngd_keys[lo] = b; ngd_keys[hi] = a; }
      }
      __syncthreads();
    }
  for (int r = tid; r < n; r += NGD_THREADS) {
    const uint64_t key = ngd_keys[r];
    const uint32_t bits = static_cast<uint32_t>(key >> 32), unit = ~static_cast<uint32_t>(key);
    if (unit >= static_cast<uint32_t>(n)) continue;           // (no live key decodes to one)
    const int64_t o = i * ld + unit;
    if (Q) Q[o] = bits < FLT_MAX_BITS ? table[r] : 0.0;
    if (rank_out) rank_out[o] = r;
    if (dunit_out) dunit_out[o] = __uint_as_float(bits);
  }
  if (Q)
    for (int64_t r = n + tid; r < ld; r += NGD_THREADS) Q[i * ld + r] = 0.0;
  if (tid == 0 && d0) {
    const uint32_t bits = static_cast<uint32_t>(ngd_keys[0] >> 32);
    d0[off + i] = bits < FLT_MAX_BITS ? __uint_as_float(bits) : -1.0f;
  }
}

}  // namespace somhip
