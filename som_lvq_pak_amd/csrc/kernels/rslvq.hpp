// kernels/rslvq.hpp -- K13: batch Robust Soft LVQ -- the posteriors of every sample over every row, the dense fp64 MFMA
// product of the posterior coefficients with the data, and the update
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "gmlvq.hpp"

namespace somhip {

// =====================================================================================
// K13: one epoch of batch RSLVQ (the definition is in include/somhip_rslvq.h).  Per chunk of samples:
//
//   distances  K1w's k_knn_dist over k_pack_samples tiles, unchanged: dist[s][storage row], the exact fp32 sum of every row.
//   posterior  k_rslvq_posterior: one wave per sample, three streams over its distance row.  The first finds the two keys
//              (own class, other classes) and with them the two maxima; the second forms exp(g - m_all) and, on the rows of
//              the sample's class, exp(g - m_own), and adds them to the two chains by a serial carry: within a stride of 64
//              rows lane 0's term first, lane 63's last, stride after stride -- one chain in row order; the third divides.
//              Q[s][j] (fp64, j the row's index, ld = 64 * row groups, zeros behind the last row), cost_s, correct_s, P(y | x).
//   sums       k_rslvq_sums: [G | c] = Q^T x [X | 1] on v_mfma_f64_16x16x4_f64, the samples as the inner dimension.
//   update     k_rslvq_update: w <- (float)(W + a * (G - c W)) over the storage tiles, in place.
//
// No floating-point atomics and no reduction whose order the definition does not name: every figure is a function of the
// data, the codebook and the shape alone.
// =====================================================================================
constexpr int RS_WAVES = 4;                   // posterior: samples (waves) of a workgroup
constexpr int RS_TILE = 64;                   // sums: prototype rows of a workgroup, and samples of a staged tile
constexpr int RS_COLS = 64;                   // sums: columns of X of a workgroup: four 16-column MFMA tiles
constexpr int RS_LDS_COLS = RS_COLS + 16;     // ... and a fifth tile whose column 0 is the ones column, which carries c
constexpr int RS_THREADS = 256;               // the update

__device__ __forceinline__ double rs_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// Steps 2 (the keys) and 3 of the definition for chunk sample i = blockIdx.x * RS_WAVES + wave (< count), run sample
// off + i, data row (first + off + i) % n_rows (first < n_rows).  dist[i][ld]: k_knn_dist's output, indexed by storage
// row; the lane walks row indices j = 64 g + lane and looks its storage row up (the identity outside patch order).
// two_s = 2.0 * (double)sigma2.  Every operation is one fp64 rounding in the order written:
//   g_j = -(double)d_j / two_s; m_all = g of the smallest distance, m_own = g of the smallest own-label distance (the
//   quotient is monotone in d, so these are the maxima); ea_j = exp(g_j - m_all), eo_j = exp(g_j - m_own) on own rows;
//   Z_all += ea_j and Z_own += eo_j in row order (a row of another class adds +0.0 to Z_own, which leaves its bits);
//   P_j = ea_j / Z_all; q_j = eo_j / Z_own - P_j on own rows, -P_j on the others;
//   cost = (m_all + log(Z_all)) - (m_own + log(Z_own)); pown = exp(-cost); correct = key_own < key_other.
// Q row i of the chunk holds ea between the second stream and the third (a lane reads back what it wrote itself).
__global__ __launch_bounds__(RS_WAVES * WAVE) void k_rslvq_posterior(CbView cb, const float *__restrict__ dist, int64_t ld, int64_t count,
                                                                      int64_t off, const int32_t *__restrict__ cb_labels,
                                                                      const int32_t *__restrict__ ds_labels, int64_t n_rows, int64_t first,
                                                                      double two_s, double *__restrict__ Q, double *__restrict__ cost_s,
                                                                      int32_t *__restrict__ correct_s, double *__restrict__ pown) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * RS_WAVES + wave;
  if (i >= count) return;                     // (no barrier in this kernel)
  const int64_t smp = off + i;
  const int32_t ls = ds_labels[(first + smp) % n_rows];
  const float *drow = dist + i * ld;
  double *qrow = Q + i * ld;

  uint64_t own = KEY_NONE, other = KEY_NONE;
  for (int64_t g = 0; g < cb.ngroups; g++) {
    const int64_t j = g * WAVE + lane;
    if (j < cb.n) {
      const uint64_t k = make_key(drow[row_of_unit(cb, static_cast<uint32_t>(j))], static_cast<uint32_t>(j));
      if (cb_labels[j] == ls) own = k < own ? k : own;
      else other = k < other ? k : other;
    }
  }
  own = wave_min_u64(own);
  other = wave_min_u64(other);
  const uint64_t best = own < other ? own : other;
  const double nd_all = -static_cast<double>(__uint_as_float(static_cast<uint32_t>(best >> 32)));
  const double nd_own = -static_cast<double>(__uint_as_float(static_cast<uint32_t>(own >> 32)));
  const double m_all = nd_all / two_s, m_own = nd_own / two_s;

  double z_all = 0.0, z_own = 0.0;
  for (int64_t g = 0; g < cb.ngroups; g++) {
    const int64_t j = g * WAVE + lane;
    double ea = 0.0, eo = 0.0;
    if (j < cb.n) {
      const double nd = -static_cast<double>(drow[row_of_unit(cb, static_cast<uint32_t>(j))]);
      const double gj = nd / two_s;
      const double ta = gj - m_all;
      ea = exp(ta);
      if (cb_labels[j] == ls) { const double to = gj - m_own; eo = exp(to); }
      qrow[j] = ea;
    }
#pragma unroll
    for (int l = 0; l < WAVE; l++) {          // the serial carry: the stride's terms in lane order, both chains side by side
      z_all += rs_readlane(ea, l);
      z_own += rs_readlane(eo, l);
    }
  }

  for (int64_t g = 0; g < cb.ngroups; g++) {
    const int64_t j = g * WAVE + lane;
    double q = 0.0;                           // behind the last row: zeros
    if (j < cb.n) {
      const double p = qrow[j] / z_all;
      q = -p;
      if (cb_labels[j] == ls) {
        const double nd = -static_cast<double>(drow[row_of_unit(cb, static_cast<uint32_t>(j))]);
        const double gj = nd / two_s;
        const double to = gj - m_own;
        const double t = exp(to) / z_own;
        q = t - p;
      }
    }
    qrow[j] = q;
  }
  if (lane == 0) {
    const double la = m_all + log(z_all), lo = m_own + log(z_own);
    const double c = la - lo;
    cost_s[smp] = c;
    pown[smp] = exp(-c);
    correct_s[smp] = own < other ? 1 : 0;
  }
}

// Step 4: [G | c] = Q^T x [X | 1] for the 64 rows j0 = 64 blockIdx.x .. j0 + 63 and the columns [64 blockIdx.y, + 64) of X,
// over the `count` samples of a chunk (chunk sample s is data row (first + s) % n_rows, first < n_rows).  4 waves, wave w
// the rows 16 w .. 16 w + 15, five 16 x 16 fp64 accumulator tiles each: four of G and one whose column 0 is c (only the
// first column block multiplies and writes it).  The samples come in data order, 64 per staged tile; the next tile's
// loads -- the Q elements and the sample rows -- are in flight in registers of their own while this one is multiplied
// (taking the Q elements four steps at a time into the registers just multiplied would fit three workgroups a CU, but
// the shorter distance to their use measured 14 % slower at 10 000 x 256).
// v_mfma_f64_16x16x4_f64 takes four samples a step: A[i][k] (lane: i = lane & 15, k = lane >> 4) = Q[s + k][j0 + 16 w + i],
// straight from the Q chunk (16 consecutive doubles per k); B[k][c] (c = lane & 15, k = lane >> 4) = (double)x_{s + k}[col]
// from LDS; D / C rows (lane >> 4) + 4 reg, column lane & 15.  Rows, columns and samples past the end are zeros, not
// branches (x + 0.0 * 0.0 leaves the bits of x).  Every chunk is a multiple of 64 samples but the last, so the groups of
// four are those of one call over the whole run: the chunk length does not change a bit.
// CONT: the accumulators start from what the chunk before left in G (k_batchmap_sums<true>'s idea).  G is [n_units][d + 1].
template <bool CONT>
__global__ __launch_bounds__(256, 2) void k_rslvq_sums(const double *__restrict__ Q, int64_t ldq, int64_t count,
                                                       const float *__restrict__ rows, int64_t n_rows, int d, int64_t first,
                                                       int64_t n_units, double *__restrict__ G) {
  __shared__ double s_b[RS_TILE * RS_LDS_COLS];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  const int64_t j0 = static_cast<int64_t>(blockIdx.x) * RS_TILE;
  const int col0 = static_cast<int>(blockIdx.y) * RS_COLS;
  const bool with_c = blockIdx.y == 0;
  const int64_t ldg = d + 1;

  f64x4 acc[5];
#pragma unroll
  for (int t = 0; t < 5; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int64_t jr = j0 + wave * 16 + kq;                    // this lane's rows: jr + 4 reg
  double *gbase = G + jr * ldg + col0 + cl;                   // ... and its element (reg, tile t): gbase[4 reg ldg + 16 t]
  if (CONT) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (jr + 4 * r >= n_units) continue;
#pragma unroll
      for (int t = 0; t < 4; t++)
        if (col0 + t * 16 + cl < d) acc[t][r] = gbase[4 * r * ldg + t * 16];
      if (with_c && cl == 0) acc[4][r] = gbase[4 * r * ldg + d];
    }
  }
  for (int e = tid; e < RS_TILE * 16; e += 256) s_b[(e >> 4) * RS_LDS_COLS + RS_COLS + (e & 15)] = 0.0;   // the fifth tile: only its
                                                                                                      // column 0 is written again
  float pre_x[16];
  double pre_a[RS_TILE / 4], pre_one = 0.0;
  const double *qcol = Q + j0 + wave * 16 + cl;
  auto fetch = [&](int64_t s0) {                              // (behind the end: zeros, no load)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int64_t s = s0 + wave * 16 + r;
      int64_t dr = first + s;
      if (dr >= n_rows) { dr -= n_rows; if (dr >= n_rows) dr %= n_rows; }
      const int col = col0 + lane;
      pre_x[r] = (s < count && col < d) ? rows[dr * d + col] : 0.0f;
    }
    if (lane < 16) pre_one = s0 + wave * 16 + lane < count ? 1.0 : 0.0;
#pragma unroll
    for (int kk = 0; kk < RS_TILE / 4; kk++) {
      const int64_t s = s0 + kk * 4 + kq;
      pre_a[kk] = s < count ? qcol[s * ldq] : 0.0;
    }
  };

  fetch(0);
  for (int64_t s0 = 0; s0 < count; s0 += RS_TILE) {
    __syncthreads();                                          // the tile before is used up
#pragma unroll
    for (int r = 0; r < 16; r++) s_b[(wave * 16 + r) * RS_LDS_COLS + lane] = static_cast<double>(pre_x[r]);
    if (lane < 16) s_b[(wave * 16 + lane) * RS_LDS_COLS + RS_COLS] = pre_one;
    double a[RS_TILE / 4];
#pragma unroll
    for (int kk = 0; kk < RS_TILE / 4; kk++) a[kk] = pre_a[kk];
    __syncthreads();
    fetch(s0 + RS_TILE);
#pragma unroll
    for (int kk = 0; kk < RS_TILE / 4; kk++) {
      const double *bp = s_b + (kk * 4 + kq) * RS_LDS_COLS + cl;
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bp[t * 16], acc[t], 0, 0, 0);
      if (with_c) acc[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bp[64], acc[4], 0, 0, 0);
    }
  }

#pragma unroll
  for (int r = 0; r < 4; r++) {
    if (jr + 4 * r >= n_units) continue;
#pragma unroll
    for (int t = 0; t < 4; t++)
      if (col0 + t * 16 + cl < d) gbase[4 * r * ldg + t * 16] = acc[t][r];
    if (with_c && cl == 0) gbase[4 * r * ldg + d] = acc[4][r];
  }
}

// Step 5, in place over the storage tiles: thread = (row group, chunk of 4 dims, lane).  With W = (double)w_j[k]:
// w_j[k] = (float)(W + a * (G[j][k] - c[j] * W)), every operation one rounding.  Every row is stepped; the padding keeps
// its zeros.
__global__ __launch_bounds__(RS_THREADS) void k_rslvq_update(CbView cb, const double *__restrict__ G, double a) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * RS_THREADS + threadIdx.x;
  const int lane = static_cast<int>(t & (WAVE - 1));
  const int64_t gq = t >> 6;
  if (gq >= cb.ngroups * cb.d4) return;
  const int64_t g = gq / cb.d4;
  const int q = static_cast<int>(gq % cb.d4);
  const int64_t row = g * WAVE + lane;
  if (row >= cb.n) return;
  const double *Gj = G + static_cast<int64_t>(unit_of_row(cb, row)) * (cb.d + 1);
  const double c = Gj[cb.d];
  float4 *cp = tile_ptr_w(cb, g, q, lane);
  const float4 w = *cp;
  float v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int k = q * 4 + j;
    if (k >= cb.d) continue;
    const double W = static_cast<double>(v[j]);
    const double cw = c * W;
    const double gg = Gj[k] - cw;
    const double step = a * gg;
    v[j] = static_cast<float>(W + step);
  }
  *cp = make_float4(v[0], v[1], v[2], v[3]);
}

}  // namespace somhip
