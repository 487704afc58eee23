// kernels/knn_wide.hpp -- K1w: exact k-NN for 9 <= knn <= 256: all distances of a chunk of samples, then a select per sample
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "scan_masked.hpp"

namespace somhip {

// =====================================================================================
// K1w: find_winner_knn (lvq_pak.c:152-221) for more neighbours than the top-K kernels
// keep in registers.  Two stages per chunk of samples:
//   distance: dist[sample][ngroups * 64] <- the exact squared distance of the sample to
//             every row (K1's arithmetic: lane = row, dims in order, sub / mul / add
//             each rounded); rows beyond cb.n inside the last group hold padding sums
//   select:   one workgroup per sample streams its distances once and keeps the knn
//             smallest keys (distance bits, ~unit: later row first on equal distance,
//             lvq_pak.c:197) in LDS
// Exact: no MFMA, no pre-filter.
// =====================================================================================

// distance stage, unmasked data: the tiling of k_scan_exact (S samples per workgroup tile, a row group per wave) with
// the sums stored instead of reduced -- for every sample the 64 lanes of a wave write 64 consecutive floats
template <int S>
__global__ __launch_bounds__(256) void k_knn_dist(CbView cb, const float4 *__restrict__ xt, int64_t count, int64_t ld,
                                                  float *__restrict__ dist) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t sb = blockIdx.x;
  const int64_t g = static_cast<int64_t>(blockIdx.y) * 4 + wave;
  if (g >= cb.ngroups) return;                // (no barrier in this kernel)
  const float4 *xtile = xt + sb * cb.d4 * S;
  float acc[S];
#pragma unroll
  for (int s = 0; s < S; s++) acc[s] = 0.0f;
  for (int q = 0; q < cb.d4; q++) {
    const float4 c = *tile_ptr(cb, g, q, lane);
#pragma unroll
    for (int s = 0; s < S; s++) {
      const float4 x = xtile[q * S + s];      // wave-uniform address
      float a = acc[s];
      a = sq_acc(a, c.x, x.x);
      a = sq_acc(a, c.y, x.y);
      a = sq_acc(a, c.z, x.z);
      a = sq_acc(a, c.w, x.w);
      acc[s] = a;
    }
  }
  float *out = dist + g * WAVE + lane;
#pragma unroll
  for (int s = 0; s < S; s++) {
    const int64_t smp = sb * S + s;
    if (smp < count) out[smp * ld] = acc[s];
  }
}

// distance stage, masked data: one sample per launch column as in K1m; only the sample's mask counts, a masked
// component is skipped, never added as zero (lvq_pak.c:179-186)
__global__ __launch_bounds__(256) void k_knn_dist_masked(CbView cb, const float *__restrict__ rows,
                                                         const uint8_t *__restrict__ mask, int64_t n_rows, int64_t first,
                                                         int64_t ld, float *__restrict__ dist) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t smp = blockIdx.y;
  const int64_t r = (first + smp) % n_rows;
  const float *x = rows + r * cb.d;
  const uint8_t *m = mask + r * cb.d;
  const int64_t g = static_cast<int64_t>(blockIdx.x) * 4 + wave;
  if (g >= cb.ngroups) return;
  float acc = 0.0f;
  for (int q = 0; q < cb.d4; q++) {
    float4 c = *tile_ptr(cb, g, q, lane);
    float cc[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      int i = q * 4 + j;
      if (i < cb.d && m[i] == 0) acc = sq_acc(acc, cc[j], x[i]);
    }
  }
  dist[smp * ld + g * WAVE + lane] = acc;
}

constexpr int KNN_WIDE_MAX = 256;      // most neighbours of the select stage (include/somhip.h: SOMHIP_KNN_MAX)
constexpr int KNN_POOL = 1024;         // keys of a sample's pool in LDS: [0, knn) the best so far, the rest candidates
constexpr int KNN_THREADS = 256;       // threads of a select workgroup = rows of a stride
static_assert(KNN_WIDE_MAX + 2 * KNN_THREADS <= KNN_POOL, "at least two strides between two flushes");

// ascending bitonic sort of the whole pool by the workgroup; ends behind a barrier
__device__ __forceinline__ void knn_pool_sort(uint64_t *pool) {
  for (int k = 2; k <= KNN_POOL; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < KNN_POOL / 2; t += KNN_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));     // the pair's element with bit j clear
        const int p = i | j;
        const uint64_t a = pool[i], b = pool[p];
        if ((a > b) == ((i & k) == 0)) { pool[i] = b; pool[p] = a; }
      }
      __syncthreads();
    }
}

// select stage: keys[sample][knn] <- the knn smallest keys of dist[sample][0, cb.n), ascending, KEY_NONE where the
// codebook has fewer rows.  A key enters the candidate part of the pool only if it is below the knn-th best of the last
// flush (strictly: keys of live rows are unique); a flush sorts the pool when the next stride of 256 rows might not fit.
// What a flush leaves in [knn, KNN_POOL) are keys of rows already seen and not among the knn best: the next
// candidates overwrite them from slot knn on, and those that stay sort behind the knn best again.
// The pool's fill is a register, the same in every thread: a stride's waves count the keys they add into cnt[stride % 3]
// (one LDS add per wave, lane slots by ballot / mbcnt), and the next stride adds that word to its fill behind the one
// barrier at its top -- no thread reads a word another may still be adding to, so the flush decision is uniform.
// Every distance is read once; worst case (every key passes: equal rows, distances falling with the row index) one
// sort per 768 rows.
__global__ __launch_bounds__(KNN_THREADS) void k_knn_select(CbView cb, const float *__restrict__ dist, int64_t ld, int knn,
                                                            uint64_t *__restrict__ keys) {
  __shared__ uint64_t pool[KNN_POOL];
  __shared__ int cnt[3];
  const int tid = threadIdx.x, lane = tid & 63;
  const float *drow = dist + static_cast<int64_t>(blockIdx.x) * ld;
  for (int i = tid; i < KNN_POOL; i += KNN_THREADS) pool[i] = KEY_NONE;
  if (tid < 3) cnt[tid] = 0;
  uint64_t thr = KEY_NONE;
  int fill = knn;                             // pool slots in use at the top of the stride
  int cur = 0, prev = 2, next = 1;            // stride % 3 and its neighbours
  // four strides of loads at a time
  for (int64_t base4 = 0; base4 < cb.n; base4 += 4 * KNN_THREADS) {
    float d[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t row = base4 + u * KNN_THREADS + tid;
      d[u] = row < cb.n ? drow[row] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int64_t base = base4 + u * KNN_THREADS;
      if (base >= cb.n) break;                // (uniform)
      __syncthreads();                        // the pool's preset; the last stride's keys and their number
      fill += cnt[prev];
      if (tid == 0) cnt[next] = 0;            // (read last at the top of the stride before this one)
      if (fill + KNN_THREADS > KNN_POOL) {
        knn_pool_sort(pool);
        thr = pool[knn - 1];
        fill = knn;
      }
      const int64_t row = base + tid;
      const uint64_t key = row < cb.n ? make_key(d[u], ~unit_of_row(cb, row)) : KEY_NONE;
      const bool pass = key < thr;
      const unsigned long long m = __ballot(pass);
      int slot0 = 0;
      if (lane == 0 && m) slot0 = atomicAdd(&cnt[cur], __popcll(m));
      slot0 = fill + __shfl(slot0, 0, WAVE);
      const int below = static_cast<int>(__builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                                  __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u)));
      if (pass) pool[slot0 + below] = key;    // fill + 256 <= KNN_POOL holds here
      prev = cur; cur = next; next = 3 - prev - cur;
    }
  }
  __syncthreads();
  knn_pool_sort(pool);
  uint64_t *out = keys + static_cast<int64_t>(blockIdx.x) * knn;
  for (int i = tid; i < knn; i += KNN_THREADS) out[i] = pool[i];
}

}  // namespace somhip
