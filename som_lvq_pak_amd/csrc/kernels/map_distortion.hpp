// kernels/map_distortion.hpp -- K1d: map distortion -- the SOM energy at a radius, per unit, from the batch map's per-unit
// sums and one more per-unit chain, on the fp64 MFMA
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "batchmap.hpp"

namespace somhip {

// =====================================================================================
// K1d: E(r) = sum_s sum_j h_r(c(s), j) |x_s - m_j|^2 without a samples x units x dim sweep.  With
// K8's hits[c] and S[c][k] and one more chain per unit, Q[c] = sum over the unit's samples of |x_s|^2:
//
//   e_j = A_j - 2 sum_k m_jk N_jk + D_j sum_k m_jk^2,      [N | D | A] = H x [S | hits | Q]
//
//   q        k_distortion_q: q[s] = |x_s|^2 in fp64, the 64 lanes of a wave over the components of a sample.
//   qsums    k_distortion_qsums: Q[u] goes on, one chain of fp64 additions over the unit's list in data order (the list is
//            the batch map's: k_batchmap_winners, k_batchmap_starts, the sort).
//   evaluate k_distortion_evaluate: the combine's product with Q in column 1 of the fifth tile; the epilogue reduces
//            against the codebook's rows and writes partials per (unit, column block), not the rows.
//   fold     k_distortion_units: the column blocks in order into e_j and scale_j; k_distortion_fold: the units into E and
//            the scale.
//
// No floating-point atomics; every order of additions is a function of the shape alone.
// =====================================================================================
constexpr int DS_THREADS = 256;               // the q pass (a wave per sample), the q sums (a wave per unit), the per-unit fold (a lane per unit)
constexpr int DS_FOLD_THREADS = 1024;         // the fold over the units: one workgroup

// q[s] = |x|^2 of data row (first + s) % n_rows (first < n_rows), s < count, in fp64: lane l of the sample's wave adds
// (double)x[k] * (double)x[k] -- exact: 48 bits -- for k = l, l + 64, ... in order from +0.0, then the 64 partials are
// folded by the xor butterfly 32, 16, 8, 4, 2, 1 (both lanes of a pair form the same sum: fp addition commutes).  The
// order depends on d alone.  One wave per sample: the rows are read once, 256 contiguous bytes per wave and step.  (Four
// samples side by side per wave measured the same: the pass runs at the rate of the memory as it is.)
__global__ __launch_bounds__(DS_THREADS) void k_distortion_q(const float *__restrict__ rows, int64_t n_rows, int d, int64_t first,
                                                             int64_t count, double *__restrict__ q) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t s = static_cast<int64_t>(blockIdx.x) * (DS_THREADS / WAVE) + (threadIdx.x >> 6);
  if (s >= count) return;                                     // (the whole wave)
  int64_t r = first + s;
  if (r >= n_rows) r %= n_rows;
  const float *x = rows + r * d;
  double acc = 0.0;
  for (int k = lane; k < d; k += WAVE) {
    const double v = static_cast<double>(x[k]);
    acc += v * v;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, WAVE);
  if (lane == 0) q[s] = acc;
}

// Q[u] += q[list[i]], i = starts[u] .. starts[u + 1] - 1 in order: the chain the pieces before this one left in Q[u] (+0.0
// before the first) goes on over this piece's samples of unit u in data order.  A unit without a sample of this piece
// keeps its bits.  One wave per unit: the lanes fetch 64 entries of the list at once (one contiguous read of the list, one
// gather of q) and the chain takes them lane by lane through v_readlane, every lane forming the same sum, while the next
// 64 are on their way.  (A lane per unit with its own list walked the lists at the rate one CU resolves scattered
// addresses: 1.04 ms at 1024 units over 1 M samples)
__device__ __forceinline__ double ds_readlane_f64(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}
__global__ __launch_bounds__(DS_THREADS) void k_distortion_qsums(const uint32_t *__restrict__ list, const uint32_t *__restrict__ starts,
                                                                 uint32_t n_units, const double *__restrict__ q, double *__restrict__ Q) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t u = blockIdx.x * (DS_THREADS / WAVE) + (threadIdx.x >> 6);
  if (u >= n_units) return;                                   // (the whole wave)
  const uint32_t lo = __builtin_amdgcn_readfirstlane(starts[u]), hi = __builtin_amdgcn_readfirstlane(starts[u + 1]);
  if (lo == hi) return;
  double acc = Q[u];
  double v = static_cast<uint64_t>(lo) + lane < hi ? q[list[static_cast<uint64_t>(lo) + lane]] : 0.0;
  for (uint64_t i = lo; i < hi; i += WAVE) {                  // (64-bit: i + 127 may pass 2^32)
    const uint64_t nx = i + WAVE + lane;
    const double next = nx < hi ? q[list[nx]] : 0.0;
    const uint64_t m = hi - i;
    if (m >= WAVE) {
#pragma unroll
      for (int j = 0; j < WAVE; j++) acc += ds_readlane_f64(v, j);
    } else {
      for (int j = 0; j < static_cast<int>(m); j++) acc += ds_readlane_f64(v, j);
    }
    v = next;
  }
  if (lane == 0) Q[u] = acc;
}

// [N | D | A] = H x [S | hits | Q] for the 64 rows of row group blockIdx.x and the columns [blockIdx.y * BM_COLS, + BM_COLS)
// of a whole map, reduced against the rows' own m_jk.  The tiling, the operand layouts, the staged tile with the next
// tile's loads in flight and the weights are k_batchmap_combine's (batchmap.hpp) written out again, and the bubble group
// skip is its rule called (bm_group_skipped); here the fifth tile carries hits in its column 0 and Q in its column 1.  Epilogue, per destination row j (lane:
// rows (lane >> 4) + 4 reg of the wave's 16, column lane & 15 of each tile): with m = m_jk read from the codebook's tiles
// (0 past the end), t_k = m * (D_j * m - 2 N_jk) and m * m (exact) are added over the lane's four tiles in order from +0.0,
// the 16 lanes of a row are folded by the xor butterfly 8, 4, 2, 1, and lane 0 of the row writes
//   pe[unit][blockIdx.y] = the partial of sum_k t_k, behind A_j in column block 0 (A_j + partial)
//   pm[unit][blockIdx.y] = the partial of sum_k m_jk^2
//   da[unit] = {D_j, A_j}                                   (column block 0)
// Nothing else is written: the codebook is read only.
template <bool GAUSS>
__global__ __launch_bounds__(256, 3) void k_distortion_evaluate(CbView cb, int ydim, const double *__restrict__ S,
                                                             const double *__restrict__ Q, float thresh, int small_map,
                                                             const double *__restrict__ table, double *__restrict__ pe,
                                                             double *__restrict__ pm, double *__restrict__ da) {
  __shared__ double s_b[BM_TILE * BM_LDS_COLS];
  __shared__ int2 s_xy[BM_TILE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  const int64_t g = blockIdx.x;
  const int col0 = static_cast<int>(blockIdx.y) * BM_COLS;
  const int d = cb.d;
  const int64_t ld = d + 1;
  const int W = 2 * cb.xdim - 1, H = 2 * ydim - 1;
  const int64_t drow = g * BM_TILE + wave * 16 + cl;
  int tx = 0, ty = 0;
  if (drow < cb.n) txty_of_row(cb, drow, tx, ty);
  int dx0 = 0, dx1 = 0, dy0 = 0, dy1 = 0;
  if (!GAUSS) bm_group_box(cb, g, dx0, dx1, dy0, dy1);
  f64x4 acc[5];
#pragma unroll
  for (int t = 0; t < 5; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int e = tid; e < BM_TILE * 16; e += 256) s_b[(e >> 4) * BM_LDS_COLS + BM_COLS + (e & 15)] = 0.0;   // the fifth tile: only its
                                                                                                      // columns 0 and 1 are ever written again

  int spx = 0, spy = 0;
  auto skipped = [&](int64_t s) -> bool { return bm_group_skipped<GAUSS>(cb, s, spx, spy, dx0, dx1, dy0, dy1, thresh); };
  auto after = [&](int64_t s) -> int64_t {                            // the first group behind s that is not skipped
    do {
      s++;
      if (++spx == cb.patch_w) { spx = 0; spy++; }
    } while (s < cb.ngroups && skipped(s));
    return s;
  };
  double pre[16], pre_h = 0.0;
  int2 pre_xy = make_int2(0, 0);
  auto fetch = [&](int64_t s) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int64_t srow = s * BM_TILE + wave * 16 + r;
      const bool valid = srow < cb.n;
      const double *sp = S + static_cast<int64_t>(valid ? unit_of_row(cb, srow) : 0u) * ld;
      const int col = col0 + lane;
      pre[r] = (valid && col < d) ? sp[col] : 0.0;
    }
    if (lane < 32) {                                                  // lane r: the count of the wave's source row r; lane 16 + r: its Q
      const int64_t srow = s * BM_TILE + wave * 16 + cl;
      const int64_t su = srow < cb.n ? static_cast<int64_t>(unit_of_row(cb, srow)) : 0;
      pre_h = srow < cb.n ? (lane < 16 ? S[su * ld + d] : Q[su]) : 0.0;
    }
    if (tid < BM_TILE) {
      const int64_t srow = s * BM_TILE + tid;
      int bx = 0, by = 0;
      if (srow < cb.n) txty_of_row(cb, srow, bx, by);
      pre_xy = make_int2(bx, by);
    }
  };

  int64_t sg = skipped(0) ? after(0) : 0;
  if (sg < cb.ngroups) fetch(sg);
  while (sg < cb.ngroups) {
    __syncthreads();                                          // the tile before is used up
#pragma unroll
    for (int r = 0; r < 16; r++) s_b[(wave * 16 + r) * BM_LDS_COLS + lane] = pre[r];
    if (lane < 32) s_b[(wave * 16 + cl) * BM_LDS_COLS + BM_COLS + kq] = pre_h;
    if (tid < BM_TILE) s_xy[tid] = pre_xy;
    __syncthreads();
    double a[BM_TILE / 4];
    if (GAUSS) {
#pragma unroll
      for (int kk = 0; kk < BM_TILE / 4; kk++) {
        const int2 b = s_xy[kk * 4 + kq];
        a[kk] = table[(static_cast<int64_t>(b.y & 1) * H + (b.y - ty + ydim - 1)) * W + (b.x - tx + cb.xdim - 1)];
      }
    }
    sg = after(sg);
    if (sg < cb.ngroups) fetch(sg);
#pragma unroll
    for (int kk = 0; kk < BM_TILE / 4; kk++) {
      const int ks = kk * 4 + kq;
      if (!GAUSS) {
        const int2 b = s_xy[ks];
        const float lsq = small_map ? lattice_sq_small(cb.topol, b.x, b.y, tx, ty) : lattice_sq(cb.topol, b.x, b.y, tx, ty);
        a[kk] = lsq <= thresh ? 1.0 : 0.0;
      }
      const double *bp = s_b + ks * BM_LDS_COLS + cl;
#pragma unroll
      for (int t = 0; t < 5; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bp[t * 16], acc[t], 0, 0, 0);
    }
  }

  const int nblk = static_cast<int>(gridDim.y);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int rl = wave * 16 + kq + 4 * r;
    const int64_t row = g * BM_TILE + rl;
    const double den = __shfl(acc[4][r], lane & 48, WAVE);           // columns 0 and 1 of the fifth tile, same rows
    const double a_j = __shfl(acc[4][r], (lane & 48) | 1, WAVE);
    double te = 0.0, tm = 0.0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int col = col0 + t * 16 + cl;
      double m = 0.0;
      if (row < cb.n && col < d) m = static_cast<double>(cb.tiles[((g * cb.d4 + (col >> 2)) * WAVE + rl) * 4 + (col & 3)]);
      const double dm = den * m;
      const double n2 = 2.0 * acc[t][r];
      const double df = dm - n2;
      te += m * df;
      tm += m * m;
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      te += __shfl_xor(te, o, WAVE);
      tm += __shfl_xor(tm, o, WAVE);
    }
    if (cl == 0 && row < cb.n) {
      const int64_t u = static_cast<int64_t>(unit_of_row(cb, row));
      pe[u * nblk + blockIdx.y] = blockIdx.y == 0 ? a_j + te : te;
      pm[u * nblk + blockIdx.y] = tm;
      if (blockIdx.y == 0) { da[2 * u] = den; da[2 * u + 1] = a_j; }
    }
  }
}

// e_j and scale_j of unit j = a lane, from the partials.  The column blocks are added in order from +0.0: e_j = sum_b
// pe[j][b] and |m_j|^2 = sum_b pm[j][b]; where D_j == 0, e_j = 0 and scale_j = 0; else scale_j = 2 * (A_j + D_j * |m_j|^2).
__global__ __launch_bounds__(DS_THREADS) void k_distortion_units(const double *__restrict__ pe, const double *__restrict__ pm,
                                                                 const double *__restrict__ da, uint32_t n_units, int nblk,
                                                                 double *__restrict__ unit_e, double *__restrict__ unit_s) {
  const uint32_t u = blockIdx.x * DS_THREADS + threadIdx.x;
  if (u >= n_units) return;
  double e = 0.0, msq = 0.0;
  for (int b = 0; b < nblk; b++) {
    e += pe[static_cast<int64_t>(u) * nblk + b];
    msq += pm[static_cast<int64_t>(u) * nblk + b];
  }
  const double den = da[2 * static_cast<int64_t>(u)], a_j = da[2 * static_cast<int64_t>(u) + 1];
  double sc = 0.0;
  if (den == 0.0) e = 0.0;
  else {
    const double t = den * msq;
    sc = 2.0 * (a_j + t);
  }
  unit_e[u] = e;
  unit_s[u] = sc;
}

// totals = {E, scale} = the sums of unit_e and unit_s.  One workgroup; thread t adds the units t, t + DS_FOLD_THREADS, ... in
// order from +0.0; the threads' sums are folded in LDS by halving (t += t + 512, 256, ... 1): a tree fixed by the number
// of units.
__global__ __launch_bounds__(DS_FOLD_THREADS) void k_distortion_fold(const double *__restrict__ unit_e, const double *__restrict__ unit_s,
                                                                     uint32_t n_units, double *__restrict__ totals) {
  __shared__ double s_e[DS_FOLD_THREADS], s_s[DS_FOLD_THREADS];
  const uint32_t tid = threadIdx.x;
  double sum_e = 0.0, sum_s = 0.0;
  for (uint32_t u = tid; u < n_units; u += DS_FOLD_THREADS) {
    sum_e += unit_e[u];
    sum_s += unit_s[u];
  }
  s_e[tid] = sum_e;
  s_s[tid] = sum_s;
  __syncthreads();
  for (uint32_t o = DS_FOLD_THREADS / 2; o >= 1; o >>= 1) {
    if (tid < o) { s_e[tid] += s_e[tid + o]; s_s[tid] += s_s[tid + o]; }
    __syncthreads();
  }
  if (tid == 0) { totals[0] = s_e[0]; totals[1] = s_s[0]; }
}

}  // namespace somhip
