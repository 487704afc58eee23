// kernels/batchmap.hpp -- K8: the batch map -- per-unit ordered fp64 sums of whole data rows, and the neighbourhood
// combine on the fp64 MFMA
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "map_quality.hpp"

namespace somhip {

// =====================================================================================
// K8: one epoch of Kohonen's batch map.  Behind the winner search of every sample against the
// frozen codebook (SOMHIP_TIE_FIRST keys):
//
//   group    k_batchmap_winners leaves win[s] (the winner, n_units for a sample without one) and idx[s] = s per sample
//            and counts hits[u] by integer atomics; k_batchmap_starts scans the counts; a stable device radix sort of
//            (win, idx) by win (the host, rocPRIM) leaves list[]: the samples of unit u at list[starts[u] ..
//            starts[u + 1]) in data order.
//   sums     k_batchmap_sums: S[u][k] = one chain of fp64 additions from +0.0 over the unit's list, S[u][dim] = hits[u].
//            k_batchmap_sums<true> continues the chains a piece of the data left in S (somhip_batchmap_accumulate).
//   combine  k_batchmap_combine: [N | D] = H x [S | hits] on v_mfma_f64_16x16x4_f64, H generated per lane, then
//            m_i[k] = (float)(N[i][k] / D[i]) into the codebook's tiles where D[i] > 0.  Its bubble group-skip rule,
//            bm_group_skipped, is stated here once for K8m's and K1d's lattice GEMMs too; the rest of the walk (fetch,
//            staging, weights, MFMA loop) is written out in each of the three kernels.
//
// No floating-point atomics: S has the same bits on every run, and the combine's order of additions over the source
// units is the storage order of the rows, four at a time inside the MFMA -- a function of the shape alone.
// =====================================================================================
constexpr int BM_THREADS = 256;               // the winners pass
constexpr int BM_SCAN_THREADS = 1024;         // the scan of the counts: one workgroup
constexpr int BM_SUM_DIMS = WAVE;             // columns of a sums workgroup: one wave, lane = column
constexpr int BM_SUM_AHEAD = 8;               // rows of a list requested ahead of the chain
constexpr int BM_TILE = 64;                   // combine: destination rows of a workgroup (a row group) and source rows of a staged tile
constexpr int BM_COLS = 64;                   // combine: numerator columns of a workgroup: four 16-column MFMA tiles
constexpr int BM_LDS_COLS = BM_COLS + 16;     // ... and a fifth tile that holds the counts column, so every workgroup has D
typedef double f64x4 __attribute__((ext_vector_type(4)));

// Per sample s of the chunk (the run's sample off + s) from keys[s][stride]: win = the winning unit, or n_units where
// nothing beat FLT_MAX; idx = the sample's number in the run; d1 (null: not wanted) = the winner's squared distance, -1
// without one; hits[win]++.
__global__ __launch_bounds__(BM_THREADS) void k_batchmap_winners(const uint64_t *__restrict__ keys, int stride, int64_t off,
                                                                 int64_t count, uint32_t n_units, uint32_t *__restrict__ win,
                                                                 uint32_t *__restrict__ idx, float *__restrict__ d1,
                                                                 uint32_t *__restrict__ hits) {
  const int64_t smp = static_cast<int64_t>(blockIdx.x) * BM_THREADS + threadIdx.x;
  if (smp >= count) return;
  const uint64_t k = keys[smp * stride];
  const uint32_t u = static_cast<uint32_t>(k);
  const bool has = static_cast<uint32_t>(k >> 32) < FLT_MAX_BITS && u < n_units;
  win[off + smp] = has ? u : n_units;
  idx[off + smp] = static_cast<uint32_t>(off + smp);
  if (d1) d1[smp] = has ? __uint_as_float(static_cast<uint32_t>(k >> 32)) : -1.0f;
  if (has) atomicAdd(hits + u, 1u);
}

// starts[u] = hits[0] + ... + hits[u - 1], u = 0 .. n_units (the last one: every sample with a winner).  One workgroup:
// every lane sums a run of units, the runs' totals are scanned in LDS.
__global__ __launch_bounds__(BM_SCAN_THREADS) void k_batchmap_starts(const uint32_t *__restrict__ hits, uint32_t n_units,
                                                                     uint32_t *__restrict__ starts) {
  __shared__ uint32_t s_part[BM_SCAN_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t per = (n_units + BM_SCAN_THREADS - 1) / BM_SCAN_THREADS;
  const uint32_t lo = min(tid * per, n_units), hi = min(lo + per, n_units);
  uint32_t sum = 0;
  for (uint32_t u = lo; u < hi; u++) sum += hits[u];
  s_part[tid] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < BM_SCAN_THREADS; o <<= 1) {
    const uint32_t v = tid >= o ? s_part[tid - o] : 0u;
    __syncthreads();
    s_part[tid] += v;
    __syncthreads();
  }
  uint32_t run = s_part[tid] - sum;
  for (uint32_t u = lo; u < hi; u++) { starts[u] = run; run += hits[u]; }
  if (tid == BM_SCAN_THREADS - 1) starts[n_units] = s_part[tid];
}

// S[u][k] for unit u = blockIdx.x and column k = blockIdx.y * BM_SUM_DIMS + lane: the chain of fp64 additions, from +0.0,
// of (double)x[k] over the unit's samples in data order (sample s is data row (first + s) % n_rows, first < n_rows);
// S[u][d] = (double)hits[u].  S is [n_units][d + 1].  The list is known, so BM_SUM_AHEAD rows are loaded -- a wave reads
// 256 contiguous bytes of each -- before their additions run in order.
// CONT: the data come in pieces and S holds what the pieces before this one left (+0.0 and a count of 0.0 before the
// first): the chain goes on from S[u][k] and the count grows by hits[u] (exact: an integer below 2^32 in fp64).  A chain
// from a stored +0.0 is the chain from +0.0, so the pieces leave the bits of one call over their rows in order.  An
// instantiation of its own: the one-call kernel keeps its code, with no load of S ahead of its chain.
template <bool CONT>
__global__ __launch_bounds__(BM_SUM_DIMS) void k_batchmap_sums(const float *__restrict__ rows, int64_t n_rows, int d,
                                                               int64_t first, const uint32_t *__restrict__ list,
                                                               const uint32_t *__restrict__ starts, double *__restrict__ S) {
  const uint32_t u = blockIdx.x;
  const int k = static_cast<int>(blockIdx.y) * BM_SUM_DIMS + static_cast<int>(threadIdx.x);
  const uint32_t lo = starts[u], hi = starts[u + 1];
  if (k > d) return;
  double *out = S + static_cast<int64_t>(u) * (d + 1) + k;
  if (k == d) { *out = CONT ? *out + static_cast<double>(hi - lo) : static_cast<double>(hi - lo); return; }
  if (CONT && lo == hi) return;                               // no sample of this piece: the chain stands
  double acc = CONT ? *out : 0.0;
  uint32_t i = lo;
  for (; hi - i >= BM_SUM_AHEAD; i += BM_SUM_AHEAD) {
    float x[BM_SUM_AHEAD];
#pragma unroll
    for (int a = 0; a < BM_SUM_AHEAD; a++) x[a] = rows[run_row(first, list[i + a], n_rows) * d + k];
#pragma unroll
    for (int a = 0; a < BM_SUM_AHEAD; a++) acc += static_cast<double>(x[a]);
  }
  for (; i < hi; i++) acc += static_cast<double>(rows[run_row(first, list[i], n_rows) * d + k]);
  *out = acc;
}

// The gaussian weights of an epoch, once per lattice offset instead of once per pair of units: table[par][dy][dx] =
// exp((double)(-dd * dd / (2.0 * r * r))) (som_rout.c:808) with dd = hexa_dist / rect_dist of a winner in a lattice row of
// parity par, (dx, dy) = the winner's position less the unit's, each offset by the map's side less one.
__global__ __launch_bounds__(BM_THREADS) void k_batchmap_gauss_table(int topol, int xdim, int ydim, float radius,
                                                                     double *__restrict__ table) {
  const int W = 2 * xdim - 1, H = 2 * ydim - 1;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * BM_THREADS + threadIdx.x;
  if (i >= 2ll * W * H) return;
  const int dx = static_cast<int>(i % W) - (xdim - 1), dy = static_cast<int>((i / W) % H) - (ydim - 1);
  const int par = static_cast<int>(i / (static_cast<int64_t>(W) * H));
  const float lsq = lattice_sq(topol, dx, par, 0, par - dy);
  const float dd = static_cast<float>(sqrt(static_cast<double>(lsq)));
  const float neg = -dd * dd;
  double den = 2.0 * static_cast<double>(radius);
  den = den * static_cast<double>(radius);
  table[i] = exp(static_cast<double>(neg) / den);
}

// the lattice box [x0, x1] x [y0, y1] that holds the units of row group g of a whole map
__device__ __forceinline__ void bm_group_box(const CbView &cb, int64_t g, int &x0, int &x1, int &y0, int &y1) {
  if (cb.patch_w) {
    x0 = static_cast<int>(g % cb.patch_w) * 8; x1 = x0 + 7;
    y0 = static_cast<int>(g / cb.patch_w) * 8; y1 = y0 + 7;
    return;
  }
  const int64_t u0 = g * WAVE, u1 = min(u0 + WAVE - 1, cb.n - 1);
  y0 = static_cast<int>(u0 / cb.xdim); y1 = static_cast<int>(u1 / cb.xdim);
  if (y0 == y1) { x0 = static_cast<int>(u0 % cb.xdim); x1 = static_cast<int>(u1 % cb.xdim); }
  else { x0 = 0; x1 = cb.xdim - 1; }
}

// The group-skip rule of the lattice GEMMs (k_batchmap_combine below, k_batchmap_combine_missing in
// kernels/batchmap_missing.hpp, k_distortion_evaluate in kernels/map_distortion.hpp), stated here alone: under bubble, source
// row group s -- in patch order the patch (spx, spy) -- is skipped where its lattice box lies wholly outside the radius of the
// destination group's box [dx0, dx1] x [dy0, dy1]; gaussian skips none.  A group skipped wrongly drops samples from a
// neighbourhood without a sound.  Uniform over the workgroup: the groups and the shape only.
template <bool GAUSS>
__device__ __forceinline__ bool bm_group_skipped(const CbView &cb, int64_t s, int spx, int spy, int dx0, int dx1, int dy0, int dy1,
                                                 float thresh) {
  if (GAUSS) return false;
  int sx0, sx1, sy0, sy1;
  if (cb.patch_w) { sx0 = spx * 8; sx1 = sx0 + 7; sy0 = spy * 8; sy1 = sy0 + 7; }
  else bm_group_box(cb, s, sx0, sx1, sy0, sy1);
  const double gx = static_cast<double>(max(0, max(sx0 - dx1, dx0 - sx1)));
  const double gy = static_cast<double>(max(0, max(sy0 - dy1, dy0 - sy1)));
  const double hx = cb.topol == 4 ? gx : fmax(0.0, gx - 0.5);     // a hexagonal row is shifted by half a unit at most
  const double least = hx * hx + (cb.topol == 4 ? 1.0 : 0.75) * gy * gy;
  return least > static_cast<double>(thresh) * 1.000001;
}

// [N | D] = H x [S | hits] and the division, for the 64 rows of row group g0 + blockIdx.x and the columns
// [blockIdx.y * BM_COLS, + BM_COLS) of a whole map: 4 waves, wave w the rows 16 w .. 16 w + 15, five 16 x 16 fp64
// accumulator tiles each (four of numerators, one whose column 0 is D).  The source units come in storage order, a row
// group (BM_TILE rows) per staged LDS tile, rows and columns past the end as zeros, the next tile's loads in flight in
// registers while this one is multiplied; v_mfma_f64_16x16x4_f64 takes four
// source rows a step: A[i][k] (lane: i = lane & 15, k = lane >> 4) = h(unit i, source k) made on the spot -- bubble: the
// membership test of the online kernels, lattice_sq <= thresh; gaussian: the epoch's table -- B[k][c] (c = lane & 15,
// k = lane >> 4) from LDS, and D / C rows (lane >> 4) + 4 reg, column lane & 15 (the f64 form's own layout).  Bubble skips
// the source groups whose lattice box lies wholly outside the radius of this group's box.  The epilogue writes
// (float)(N / D) into the tiles where D > 0; it has read S only, so writing in place is safe.
template <bool GAUSS>
__global__ __launch_bounds__(256, 3) void k_batchmap_combine(CbView cb, int ydim, const double *__restrict__ S, float thresh,
                                                          int small_map, const double *__restrict__ table, int64_t g0) {
  __shared__ double s_b[BM_TILE * BM_LDS_COLS];
  __shared__ int2 s_xy[BM_TILE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
  const int kq = lane >> 4, cl = lane & 15;
  const int64_t g = g0 + blockIdx.x;
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
                                                                                                      // column 0 is ever written again

  // The walk over the source groups that are not skipped (uniform over the workgroup: g, the group and the shape only).
  // In patch order the group's patch coordinates are counted along, not divided out.
  int spx = 0, spy = 0;
  auto skipped = [&](int64_t s) -> bool { return bm_group_skipped<GAUSS>(cb, s, spx, spy, dx0, dx1, dy0, dy1, thresh); };
  auto after = [&](int64_t s) -> int64_t {                            // the first group behind s that is not skipped
    do {
      s++;
      if (++spx == cb.patch_w) { spx = 0; spy++; }
    } while (s < cb.ngroups && skipped(s));
    return s;
  };
  // A tile on its way from S to LDS, in registers: the loads of the next tile are issued before the MFMAs of this one.
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
    if (lane < 16) {                                                  // lane r: the count of the wave's source row r
      const int64_t srow = s * BM_TILE + wave * 16 + lane;
      pre_h = srow < cb.n ? S[static_cast<int64_t>(unit_of_row(cb, srow)) * ld + d] : 0.0;
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
    if (lane < 16) s_b[(wave * 16 + lane) * BM_LDS_COLS + BM_COLS] = pre_h;
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
      const double *bp = s_b + ks * BM_LDS_COLS + cl;
#pragma unroll
      for (int t = 0; t < 5; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], bp[t * 16], acc[t], 0, 0, 0);
    }
  }

#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int rl = wave * 16 + kq + 4 * r;
    const int64_t row = g * BM_TILE + rl;
    const double den = __shfl(acc[4][r], lane & 48, WAVE);    // column 0 of the fifth tile, same rows
    if (row >= cb.n || !(den > 0.0)) continue;                // no sample in the neighbourhood: the row keeps its bits
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int col = col0 + t * 16 + cl;
      if (col < d) cb.tiles[((g * cb.d4 + (col >> 2)) * WAVE + rl) * 4 + (col & 3)] = static_cast<float>(acc[t][r] / den);
    }
  }
}

}  // namespace somhip
