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
//   sums       k_grlvq_sums: K9's chain of xi * (double)x[k] and, in the same lane, the chain of xi * ((double)x[k] - (double)w[k])^2.
//   relevance  k_grlvq_relevance: G[k] = one chain over the rows in unit order of (Rp[j][k] - Rm[j][k]).
//   update     k_grlvq_update: w <- (float)(W + (a * (double)lambda[k]) * ((Sp - sp W) - (Sm - sm W))), in place.
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

// Step 4 with the relevance chain.  K9's k_glvq_sums -- one wave per (prototype u = blockIdx.x, 64 columns, role =
// blockIdx.z), lane = column k, AHEAD (GLVQ_SUM_AHEAD) entries requested ahead -- with two accumulators per lane: S[role][u][k] as
// there (column d the chain over xi, column d + 1 of role + the chain over f into cost[u]), and for k < d
// R[role][u][k] = the chain of fp64 additions from +0.0 over the same list of  xi * (td * td),  td = (double)x_s[k] -
// (double)w_u[k]: a subtraction, two multiplications and an addition, each rounded.  w_u[k] is read once from the storage
// tiles.  S is [2][n_units][d + 1], R is [2][n_units][d].
// (A template, as the two kernels below: the compiler emits a template where it is first used, behind every kernel the
// library had, so those keep their places in the code object as well as their code.)
template <int AHEAD>
__global__ __launch_bounds__(BM_SUM_DIMS) void k_grlvq_sums(CbView cb, const float *__restrict__ rows, int64_t n_rows, int64_t first,
                                                            int64_t n, const uint32_t *__restrict__ list,
                                                            const uint32_t *__restrict__ starts, const double *__restrict__ xi,
                                                            const double *__restrict__ f, double *__restrict__ S,
                                                            double *__restrict__ R, double *__restrict__ cost) {
  const uint32_t u = blockIdx.x, role = blockIdx.z;
  const uint32_t n_units = static_cast<uint32_t>(cb.n);
  const int d = cb.d;
  const int k = static_cast<int>(blockIdx.y) * BM_SUM_DIMS + static_cast<int>(threadIdx.x);
  if (k > d + 1 || (k == d + 1 && role != 0)) return;
  const uint32_t *lst = list + static_cast<int64_t>(role) * n;
  const uint32_t *st = starts + static_cast<int64_t>(role) * (n_units + 1);
  const double *wt = k == d + 1 ? f : xi + static_cast<int64_t>(role) * n;
  const uint32_t lo = st[u], hi = st[u + 1];
  double W = 0.0;
  if (k < d) {
    const int64_t row = row_of_unit(cb, u);
    const float *tile = reinterpret_cast<const float *>(tile_ptr(cb, row >> 6, k >> 2, static_cast<int>(row & 63)));
    W = static_cast<double>(tile[k & 3]);
  }
  auto elem = [&](uint32_t s) -> float {
    if (k >= d) return 1.0f;
    int64_t r = first + static_cast<int64_t>(s);
    if (r >= n_rows) { r -= n_rows; if (r >= n_rows) r %= n_rows; }
    return rows[r * d + k];
  };
  double acc = 0.0, rel = 0.0;
  uint32_t i = lo;
  for (; hi - i >= AHEAD; i += AHEAD) {
    float x[AHEAD];
    double w[AHEAD];
#pragma unroll
    for (int a = 0; a < AHEAD; a++) {
      const uint32_t s = lst[i + a];
      w[a] = wt[s];
      x[a] = elem(s);
    }
#pragma unroll
    for (int a = 0; a < AHEAD; a++) {
      const double xd = static_cast<double>(x[a]);
      const double p = w[a] * xd;
      acc += p;
      const double td = xd - W;
      const double tt = td * td;
      const double pr = w[a] * tt;
      rel += pr;
    }
  }
  for (; i < hi; i++) {
    const uint32_t s = lst[i];
    const double xd = static_cast<double>(elem(s));
    const double ws = wt[s];
    const double p = ws * xd;
    acc += p;
    const double td = xd - W;
    const double tt = td * td;
    const double pr = ws * tt;
    rel += pr;
  }
  if (k == d + 1) { cost[u] = acc; return; }
  S[(static_cast<int64_t>(role) * n_units + u) * (d + 1) + k] = acc;
  if (k < d) R[(static_cast<int64_t>(role) * n_units + u) * d + k] = rel;
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

// Step 6, in place over the storage tiles: K9's k_glvq_update with the component's relevance in the step.  With
// W = (double)w_j[k]: g = (Sp[j][k] - sp[j] * W) - (Sm[j][k] - sm[j] * W), w_j[k] = (float)(W + (a * (double)lambda[k]) * g).
// lam is the float4[d4] tile of the search, read as floats.  A row no sample chose in either role keeps its bits; so does
// the padding.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_grlvq_update(CbView cb, const double *__restrict__ S, const uint32_t *__restrict__ hits,
                                                               const float *__restrict__ lam, double a) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * THREADS + threadIdx.x;
  const int lane = static_cast<int>(t & (WAVE - 1));
  const int64_t gq = t >> 6;
  if (gq >= cb.ngroups * cb.d4) return;
  const int64_t g = gq / cb.d4;
  const int q = static_cast<int>(gq % cb.d4);
  const int64_t row = g * WAVE + lane;
  if (row >= cb.n) return;
  const uint32_t u = unit_of_row(cb, row);
  const uint32_t n_units = static_cast<uint32_t>(cb.n);
  if (hits[u] == 0 && hits[n_units + u] == 0) return;
  const int64_t ld = cb.d + 1;
  const double *Sp = S + static_cast<int64_t>(u) * ld, *Sm = S + (static_cast<int64_t>(n_units) + u) * ld;
  const double sp = Sp[cb.d], sm = Sm[cb.d];
  float4 *cp = tile_ptr_w(cb, g, q, lane);
  const float4 c = *cp;
  float v[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int k = q * 4 + j;
    if (k >= cb.d) continue;
    const double W = static_cast<double>(v[j]);
    const double pw = sp * W, mw = sm * W;
    const double gp = Sp[k] - pw, gm = Sm[k] - mw;
    const double gg = gp - gm;
    const double al = a * static_cast<double>(lam[k]);
    const double step = al * gg;
    v[j] = static_cast<float>(W + step);
  }
  *cp = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace somhip
