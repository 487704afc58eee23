// kernels/batchmap_missing.hpp -- K8m: the batch map over data with missing values -- per-unit ordered fp64 sums that skip
// masked components and count the known ones per component, and the combine with a denominator per component
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "batchmap.hpp"

namespace somhip {

// =====================================================================================
// K8m: one epoch of the batch map where a sample may leave components out (the definition is in
// include/somhip_batchmap_missing.h).  The group stage is K8's (the winners come from the masked search); new are
//
//   sums     k_batchmap_sums_missing: S[u][k] = the chain of fp64 additions over the unit's samples that know component k,
//            C[u][k] = how many they are.
//   combine  k_batchmap_combine_missing: [N | D] = H x [S | C] on v_mfma_f64_16x16x4_f64 with value tiles and count tiles of
//            the same columns side by side, then m_i[k] = (float)(N[i][k] / D[i][k]) where D[i][k] > 0.
//
// The state is [S | C] as units x 2 dim doubles, C following S per unit: unit u's sums at [u * 2 dim, + dim), its counts
// at [u * 2 dim + dim, + dim).  On data without masks C[u][k] = hits[u] for every k and both kernels leave K8's bits.
// =====================================================================================
constexpr int BMM_COLS = 32;                  // combine: value columns of a workgroup; the same 32 columns of counts beside them
constexpr int BMM_LDS_COLS = 2 * BMM_COLS + 16;   // ... a staged row: [32 S | 32 C], padded to K8's stride (the same bank pattern)

// S[u][k] and C[u][k] for unit u = blockIdx.x and column k = blockIdx.y * BM_SUM_DIMS + lane, k_batchmap_sums's shape: the
// chain of fp64 additions, from +0.0, of (double)x[k] over the unit's samples in data order whose mask[k] is 0, and their
// number.  mask (null: every component is known) lies as rows does, one byte a component: a wave reads 64 contiguous
// bytes of it beside the row's 256.  A masked component is skipped by a select on the accumulator -- the stored value is
// loaded, converted and added, and the result dropped, so nothing of it is left, a NaN included.
// CONT: the chain and the count go on from what the pieces before left in the state (k_batchmap_sums<true>'s way).
template <bool CONT>
__global__ __launch_bounds__(BM_SUM_DIMS) void k_batchmap_sums_missing(const float *__restrict__ rows, const uint8_t *__restrict__ mask,
                                                                       int64_t n_rows, int d, int64_t first,
                                                                       const uint32_t *__restrict__ list,
                                                                       const uint32_t *__restrict__ starts, double *__restrict__ S) {
  const uint32_t u = blockIdx.x;
  const int k = static_cast<int>(blockIdx.y) * BM_SUM_DIMS + static_cast<int>(threadIdx.x);
  const uint32_t lo = starts[u], hi = starts[u + 1];
  if (k >= d) return;
  double *out = S + static_cast<int64_t>(u) * (2 * d) + k;
  if (CONT && lo == hi) return;                               // no sample of this piece: the chain and the count stand
  double acc = CONT ? out[0] : 0.0;
  uint32_t cnt = 0;
  uint32_t i = lo;
  for (; hi - i >= BM_SUM_AHEAD; i += BM_SUM_AHEAD) {
    float x[BM_SUM_AHEAD];
    uint8_t m[BM_SUM_AHEAD];
#pragma unroll
    for (int a = 0; a < BM_SUM_AHEAD; a++) {
      const int64_t at = run_row(first, list[i + a], n_rows) * d + k;
      x[a] = rows[at];
      m[a] = mask ? mask[at] : static_cast<uint8_t>(0);
    }
#pragma unroll
    for (int a = 0; a < BM_SUM_AHEAD; a++) {
      const double next = acc + static_cast<double>(x[a]);
      acc = m[a] ? acc : next;
      cnt += m[a] ? 0u : 1u;
    }
  }
  for (; i < hi; i++) {
    const int64_t at = run_row(first, list[i], n_rows) * d + k;
    const bool known = !(mask && mask[at]);
    const double next = acc + static_cast<double>(rows[at]);
    acc = known ? next : acc;
    cnt += known ? 1u : 0u;
  }
  out[0] = acc;
  out[d] = CONT ? out[d] + static_cast<double>(cnt) : static_cast<double>(cnt);   // (exact: integers below 2^32 in fp64)
}

// [N | D] = H x [S | C] and the division per component, for the 64 rows of row group g0 + blockIdx.x and the columns
// [blockIdx.y * BMM_COLS, + BMM_COLS) of a whole map.  k_batchmap_combine's walk, staging and weights written out again (see
// there), its group-skip rule called (bm_group_skipped, kernels/batchmap.hpp), with four accumulator tiles a wave: tiles 0, 1 the numerators of 32 columns, tiles 2, 3 the denominators of the
// same columns.  A staged row is [32 S | 32 C]: lanes 0 .. 31 fetch the sums, lanes 32 .. 63 the counts.  N and D of an
// element lie in the same lane and register of their tiles (the C / D layout of the f64 MFMA), so the division needs no
// exchange between lanes.  D[i][k] is accumulated by the very sequence of MFMAs that K8 accumulates D[i] by: where
// C[j][k] = hits[j] it has K8's bits.  A component with D[i][k] == 0 keeps its bits.
template <bool GAUSS>
__global__ __launch_bounds__(256, 3) void k_batchmap_combine_missing(CbView cb, int ydim, const double *__restrict__ S, float thresh,
                                                                     int small_map, const double *__restrict__ table, int64_t g0) {
  __shared__ double s_b[BM_TILE * BMM_LDS_COLS];
  __shared__ int2 s_xy[BM_TILE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  const int64_t g = g0 + blockIdx.x;
  const int col0 = static_cast<int>(blockIdx.y) * BMM_COLS;
  const int d = cb.d;
  const int64_t ld = 2 * static_cast<int64_t>(d);
  const int W = 2 * cb.xdim - 1, H = 2 * ydim - 1;
  const int64_t drow = g * BM_TILE + wave * 16 + cl;
  int tx = 0, ty = 0;
  if (drow < cb.n) txty_of_row(cb, drow, tx, ty);
  int dx0 = 0, dx1 = 0, dy0 = 0, dy1 = 0;
  if (!GAUSS) bm_group_box(cb, g, dx0, dx1, dy0, dy1);
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};

  int spx = 0, spy = 0;
  auto skipped = [&](int64_t s) -> bool { return bm_group_skipped<GAUSS>(cb, s, spx, spy, dx0, dx1, dy0, dy1, thresh); };
  auto after = [&](int64_t s) -> int64_t {
    do {
      s++;
      if (++spx == cb.patch_w) { spx = 0; spy++; }
    } while (s < cb.ngroups && skipped(s));
    return s;
  };
  // A tile on its way from the state to LDS, in registers.  Lane l < 32: S[.][col0 + l]; lane l >= 32: C[.][col0 + l - 32].
  const int col = col0 + (lane & (BMM_COLS - 1));
  const int64_t at = lane < BMM_COLS ? col : d + col;
  double pre[16];
  int2 pre_xy = make_int2(0, 0);
  auto fetch = [&](int64_t s) {
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int64_t srow = s * BM_TILE + wave * 16 + r;
      const bool valid = srow < cb.n;
      const double *sp = S + static_cast<int64_t>(valid ? unit_of_row(cb, srow) : 0u) * ld;
      pre[r] = (valid && col < d) ? sp[at] : 0.0;
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
    for (int r = 0; r < 16; r++) s_b[(wave * 16 + r) * BMM_LDS_COLS + lane] = pre[r];
    if (tid < BM_TILE) s_xy[tid] = pre_xy;
    __syncthreads();
    double a[BM_TILE / 4];
    if (GAUSS) {                                              // the tile's weights, asked for ahead of the next tile's rows
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
      const double *bp = s_b + ks * BMM_LDS_COLS + cl;
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bp[t * 16], acc[t], 0, 0, 0);
    }
  }

#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int rl = wave * 16 + kq + 4 * r;
    const int64_t row = g * BM_TILE + rl;
    if (row >= cb.n) continue;
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const int c = col0 + t * 16 + cl;
      const double den = acc[2 + t][r];                       // the same lane and register: the same element of D
      if (c < d && den > 0.0)                                 // no sample that knows it in the neighbourhood: the component keeps its bits
        cb.tiles[((g * cb.d4 + (c >> 2)) * WAVE + rl) * 4 + (c & 3)] = static_cast<float>(acc[t][r] / den);
    }
  }
}

}  // namespace somhip
