// kernels/grlvq.hpp -- K11: batch GRLVQ -- the class-wise exact winner search under the relevance-weighted metric, the
// per-prototype ordered fp64 sums with the relevance chain beside them, the ordered reduction of the relevance gradient
// over the prototypes, and the weighted update
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "glvq.hpp"

namespace somhip {

// =====================================================================================
// K11: one epoch of batch GRLVQ (the definition is in include/somhip.h).
//
//   search     k_scan_class_weighted over every row: K9's class-wise scan with d_lambda = sum_k lambda[k] (c[k] - x[k])^2 as
//              a chain of four separately rounded fp32 operations per component.  Only this direct route exists: the
//              pre-filters behind the top-8 lists are unweighted.
//   terms      K9's k_glvq_terms, K8's k_batchmap_starts and the stable sort, unchanged.
//   sums       k_grlvq_sums: K9's chain of xi * (double)x[k] and, in the same lane, the chain of xi * ((double)x[k] - (double)w[k])^2:
//              K9's body glvq_sums_chain (kernels/glvq.hpp) with its relevance flag.
//   relevance  k_grlvq_relevance: G[k] = one chain over the rows in unit order of (Rp[j][k] - Rm[j][k]).
//   update     k_grlvq_update: w <- (float)(W + (a * (double)lambda[k]) * ((Sp - sp W) - (Sm - sm W))), in place: K9's body
//              glvq_update_tiles (kernels/glvq.hpp) with the relevance in the step factor.
//
// No floating-point atomics anywhere.
// =====================================================================================
constexpr int GRLVQ_RED_AHEAD = 16;           // rows requested ahead of the reduction's chain

// The weighted distance chain: t = c - x (sq_acc's orientation), u = l * t, p = u * t, acc + p; four roundings, no
// contraction.  With l == 1.0f, u is t and the chain is sq_acc bit for bit.
__device__ __forceinline__ float sq_acc_weighted(float acc, float c, float x, float l) {
  float t = c - x;
  float u = l * t;
  float p = u * t;
  return acc + p;
}

// K9's k_scan_class (kernels/glvq.hpp) under d_lambda: the same lanes, row groups, register tiles, labels, epilogue and
// keys; lam is the relevance vector as float4[d4], padded with zeros, read at a wave-uniform address beside the sample
// tile, so it lives in scalar registers.  A kernel of its own: k_scan_class keeps its code.
template <int S, int R>
__global__ __launch_bounds__(256) void k_scan_class_weighted(CbView cb, const float4 *__restrict__ xt, const float4 *__restrict__ lam,
                                                             int64_t count, const int32_t *__restrict__ cb_labels,
                                                             const int32_t *__restrict__ ds_labels, int64_t n_rows, int64_t first,
                                                             int64_t base, uint64_t *__restrict__ keys2) {
  __shared__ uint64_t red[4][S][2];
  __shared__ int32_t s_lab[S];
  __shared__ int64_t s_smp[S];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t sb = blockIdx.x;
  const int64_t g0 = (static_cast<int64_t>(blockIdx.y) * 4 + wave) * R;
  const float4 *xtile = xt + sb * cb.d4 * S;

  if (threadIdx.x < S) {
    const int64_t j = sb * S + threadIdx.x;
    int64_t smp = -1;
    int32_t lab = 0;
    if (j < count) {
      smp = base + j;
      lab = ds_labels[(first + smp) % n_rows];
    }
    s_smp[threadIdx.x] = smp;
    s_lab[threadIdx.x] = lab;
  }

  bool live[R];
  uint32_t unit[R];
  int32_t lab[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int64_t row = (g0 + r) * WAVE + lane;
    live[r] = (g0 + r) < cb.ngroups && row < cb.n;
    unit[r] = live[r] ? unit_of_row(cb, row) : 0u;
    lab[r] = live[r] ? cb_labels[unit[r]] : 0;
  }

  float acc[R][S];
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int s = 0; s < S; s++) acc[r][s] = 0.0f;

  if (g0 < cb.ngroups) {
    for (int q = 0; q < cb.d4; q++) {
      float4 c[R];
#pragma unroll
      for (int r = 0; r < R; r++) {
        const int64_t g = g0 + r < cb.ngroups ? g0 + r : cb.ngroups - 1;
        c[r] = *tile_ptr(cb, g, q, lane);
      }
      const float4 l = lam[q];                      // wave-uniform address
#pragma unroll
      for (int s = 0; s < S; s++) {
        const float4 x = xtile[q * S + s];          // wave-uniform address
#pragma unroll
        for (int r = 0; r < R; r++) {
          float a = acc[r][s];
          a = sq_acc_weighted(a, c[r].x, x.x, l.x);
          a = sq_acc_weighted(a, c[r].y, x.y, l.y);
          a = sq_acc_weighted(a, c[r].z, x.z, l.z);
          a = sq_acc_weighted(a, c[r].w, x.w, l.w);
          acc[r][s] = a;
        }
      }
    }
  }
  __syncthreads();                                  // the tile's labels are in LDS

#pragma unroll
  for (int s = 0; s < S; s++) {
    const int32_t ls = s_lab[s];
    uint64_t own = KEY_NONE, other = KEY_NONE;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const uint64_t k = live[r] ? make_key(acc[r][s], unit[r]) : KEY_NONE;
      const bool mine = lab[r] == ls;
      const uint64_t ko = mine ? k : KEY_NONE, kx = mine ? KEY_NONE : k;
      own = ko < own ? ko : own;
      other = kx < other ? kx : other;
    }
    own = wave_min_u64(own);
    other = wave_min_u64(other);
    if (lane == 0) { red[wave][s][0] = own; red[wave][s][1] = other; }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 2 * S; e += blockDim.x) {
    const int s = e >> 1, role = e & 1;
    const int64_t smp = s_smp[s];
    if (smp < 0) continue;
    uint64_t b = red[0][s][role];
#pragma unroll
    for (int w = 1; w < 4; w++) b = red[w][s][role] < b ? red[w][s][role] : b;
    if (b != KEY_NONE)
      atomicMin(reinterpret_cast<unsigned long long *>(keys2 + 2 * smp + role), static_cast<unsigned long long>(b));
  }
}

// Step 4 with the relevance chain: K9's sums body (glvq_sums_chain, kernels/glvq.hpp) with RELEVANCE -- the second
// accumulator per lane, w_u[k] from the storage tiles, R beside S -- in one call over the data, AHEAD (GLVQ_SUM_AHEAD) entries
// requested ahead.  S is [2][n_units][d + 1], R is [2][n_units][d].
template <int AHEAD>
__global__ __launch_bounds__(BM_SUM_DIMS) void k_grlvq_sums(CbView cb, const float *__restrict__ rows, int64_t n_rows, int64_t first,
                                                            int64_t n, const uint32_t *__restrict__ list,
                                                            const uint32_t *__restrict__ starts, const double *__restrict__ xi,
                                                            const double *__restrict__ f, double *__restrict__ S,
                                                            double *__restrict__ R, double *__restrict__ cost) {
  glvq_sums_chain<false, true, AHEAD>(&cb, rows, n_rows, cb.d, first, n, static_cast<uint32_t>(cb.n), list, starts, xi, f, S, R, cost);
}

// Step 5: lane = component k, G[k] = one chain of fp64 additions from +0.0 over the rows j = 0 .. n_units - 1 in unit order
// of (Rp[j][k] - Rm[j][k]): a subtraction, then an addition.  The rows are known, so AHEAD (GRLVQ_RED_AHEAD) of them are requested
// before their additions run; a wave reads 512 contiguous bytes of either role per row.
template <int AHEAD>
__global__ __launch_bounds__(WAVE) void k_grlvq_relevance(const double *__restrict__ R, uint32_t n_units, int d, double *__restrict__ G) {
  const int k = static_cast<int>(blockIdx.x) * WAVE + static_cast<int>(threadIdx.x);
  if (k >= d) return;
  const double *Rp = R + k, *Rm = R + static_cast<int64_t>(n_units) * d + k;
  double acc = 0.0;
  uint32_t j = 0;
  for (; n_units - j >= AHEAD; j += AHEAD) {
    double p[AHEAD], m[AHEAD];
#pragma unroll
    for (int a = 0; a < AHEAD; a++) {
      p[a] = Rp[static_cast<int64_t>(j + a) * d];
      m[a] = Rm[static_cast<int64_t>(j + a) * d];
    }
#pragma unroll
    for (int a = 0; a < AHEAD; a++) {
      const double t = p[a] - m[a];
      acc += t;
    }
  }
  for (; j < n_units; j++) {
    const double t = Rp[static_cast<int64_t>(j) * d] - Rm[static_cast<int64_t>(j) * d];
    acc += t;
  }
  G[k] = acc;
}

// Step 6, in place over the storage tiles: K9's update body (glvq_update_tiles, kernels/glvq.hpp) with the component's
// relevance in the step: w_j[k] = (float)(W + (a * (double)lambda[k]) * g).  lam is the float4[d4] tile of the search, read as
// floats.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_grlvq_update(CbView cb, const double *__restrict__ S, const uint32_t *__restrict__ hits,
                                                               const float *__restrict__ lam, double a) {
  glvq_update_tiles<THREADS, true>(cb, S, hits, lam, a);
}

}  // namespace somhip
