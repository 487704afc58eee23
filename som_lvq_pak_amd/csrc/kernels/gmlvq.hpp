// kernels/gmlvq.hpp -- K12: batch GMLVQ -- the fp64 projection of rows by a matrix Omega, the update of the rows through
// Omega^T Omega, and the ordered block-wise gradient of Omega with its reduction over the blocks
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "grlvq.hpp"

namespace somhip {

// =====================================================================================
// K12: one epoch of batch GMLVQ (the definition is in include/somhip.h).
//
//   project   k_gmlvq_project: y[r] = (float)(the fp64 FMA chain over k of omega[r][k] * z[k]) for every sample and every
//             codebook row, written where the search reads: sample tiles and storage tiles of m columns.
//   search    K9's k_scan_class, unchanged, on those tiles (the metric is the plain squared distance in m dimensions).
//   terms     K9's k_glvq_terms, K8's k_batchmap_starts and the stable sort, unchanged.
//   sums      K9's k_glvq_sums, unchanged, on the original rows.
//   gradient  k_gmlvq_omega_grad: per block of GMLVQ_BLOCK samples and element (r, k) one chain in data order;
//             k_gmlvq_omega_reduce: one chain over the blocks per element.
//   update    k_gmlvq_update: w <- (float)(W + a * (Omega^T (Omega g))[k]), both products ordered chains, in place; g is
//             K9's glvq_step_g (kernels/glvq.hpp).
//
// No floating-point atomics anywhere.
// =====================================================================================
constexpr int GMLVQ_BLOCK = 4096;             // samples of a gradient block: part of the definition
constexpr int GMLVQ_RT = 8;                   // rows r of Omega per lane (projection) and per thread (gradient)
constexpr int GMLVQ_BATCH = 32;               // samples whose coefficients a gradient workgroup forms at once (256 / GMLVQ_RT)
constexpr int GMLVQ_AHEAD = 8;                // entries requested ahead of a chain
constexpr int GMLVQ_THREADS = 256;

// element (row, r) of storage tiles [groups][d4][64][4] / of sample tiles [sb][d4][S][4], as a float index
__device__ __forceinline__ int64_t gmlvq_tile_at(int64_t row, int r, int d4, int width) {
  return (((row / width) * d4 + (r >> 2)) * width + (row % width)) * 4 + (r & 3);
}

// Step 2.  Lane = row z (run sample blockIdx.x * 64 + lane: data row (first + z) % n_rows, first < n_rows; or, with rows
// null, storage row z of src), wave = RT rows of Omega: acc_r = fma((double)omega[r][k], (double)z[k], acc_r) from +0.0 in
// dimension order, omega at a wave-uniform address; the row is read once per RT outputs.  y[r] = (float)acc_r goes to
//   xt    (sample tiles [sb][d4m][S][4]: k_pack_samples' layout; the padding -- r >= m, samples behind count -- zero),
//   vt    (storage tiles [group][d4m][64][4] in src's row order; the padding zero),
//   flat  (row-major [count][m]; a codebook's rows by unit),
// whichever are given.
template <int S, int RT>
__global__ __launch_bounds__(256) void k_gmlvq_project(const float *__restrict__ om, int dim, int m, int d4m, const float *__restrict__ rows,
                                                       int64_t n_rows, int64_t first, CbView src, int64_t count, float *__restrict__ xt,
                                                       float *__restrict__ vt, float *__restrict__ flat) {
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int r0 = (static_cast<int>(blockIdx.y) * 4 + wave) * RT;
  if (r0 >= d4m * 4) return;
  const int64_t z = static_cast<int64_t>(blockIdx.x) * WAVE + lane;
  const bool live = z < count;
  const float *orow[RT];
#pragma unroll
  for (int i = 0; i < RT; i++) orow[i] = om + static_cast<int64_t>(r0 + i < m ? r0 + i : m - 1) * dim;
  const float *xrow = nullptr;
  if (rows) xrow = rows + ((first + (live ? z : count - 1)) % n_rows) * dim;
  double acc[RT];
#pragma unroll
  for (int i = 0; i < RT; i++) acc[i] = 0.0;
  const int d4 = (dim + 3) >> 2;
  for (int q = 0; q < d4; q++) {
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (rows) {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (q * 4 + j < dim) x[j] = xrow[q * 4 + j];
    } else {
      const float4 c = *tile_ptr(src, blockIdx.x, q, lane);
      x[0] = c.x; x[1] = c.y; x[2] = c.z; x[3] = c.w;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int k = q * 4 + j;
      if (k >= dim) break;
      const double xd = static_cast<double>(x[j]);
#pragma unroll
      for (int i = 0; i < RT; i++) acc[i] = __builtin_fma(static_cast<double>(orow[i][k]), xd, acc[i]);
    }
  }
  const int64_t padded = (count + S - 1) / S * S;
#pragma unroll
  for (int i = 0; i < RT; i++) {
    const int r = r0 + i;
    if (r >= d4m * 4) break;
    const float y = live && r < m ? static_cast<float>(acc[i]) : 0.0f;
    if (xt && z < padded) xt[gmlvq_tile_at(z, r, d4m, S)] = y;
    if (vt) vt[gmlvq_tile_at(z, r, d4m, WAVE)] = y;
    if (flat && live && r < m) flat[(rows ? z : static_cast<int64_t>(unit_of_row(src, z))) * m + r] = y;
  }
}

// Step 7, one block of samples.  Workgroup = (256 columns k, RT rows r of Omega from blockIdx.y * RT, sample block
// blockIdx.z), thread = column k with RT chains in registers.  The block is walked in data order in batches of
// GMLVQ_BATCH samples: first the 256 threads form the batch's coefficients, one (sample, r) each,
//   A = xi+ * ((double)y_s[r] - (double)v_i+[r]),  C = xi- * ((double)y_s[r] - (double)v_i-[r])
// (y from the projected sample tiles xt, v gathered from the projected storage tiles of pv) into LDS, with the batch's
// data rows and winners; then every thread walks the batch, AHEAD entries -- x_s[k], w_i+[k], w_i-[k], gathered through
// tile_ptr's layout -- requested ahead:  tp = (double)x - (double)w+,  acc = acc + A * tp;  tm = (double)x - (double)w-,
// acc = acc - C * tm,  every operation one rounding.  part[block][r][k] = acc.  A sample without both winners (win ==
// n_units; the entry points' checks leave none) is passed over.
template <int RT, int AHEAD>
__global__ __launch_bounds__(GMLVQ_THREADS) void k_gmlvq_omega_grad(CbView cb, CbView pv, const float *__restrict__ rows, int64_t n_rows,
                                                                    int64_t first, int64_t n, const float *__restrict__ xt,
                                                                    const uint32_t *__restrict__ win, const double *__restrict__ xi,
                                                                    double *__restrict__ part) {
  constexpr int B = GMLVQ_THREADS / RT;
  static_assert(B == GMLVQ_BATCH && B % AHEAD == 0, "one coefficient per thread and batch");
  __shared__ double s_a[B][RT], s_c[B][RT];
  __shared__ int64_t s_row[B], s_wp[B], s_wm[B];
  __shared__ int s_ok[B];
  const int dim = cb.d, m = pv.d;
  const uint32_t n_units = static_cast<uint32_t>(cb.n);
  const int tid = threadIdx.x;
  const int k = static_cast<int>(blockIdx.x) * GMLVQ_THREADS + tid;
  const int r0 = static_cast<int>(blockIdx.y) * RT;
  const int64_t s0 = static_cast<int64_t>(blockIdx.z) * GMLVQ_BLOCK;
  const int64_t s1 = s0 + GMLVQ_BLOCK < n ? s0 + GMLVQ_BLOCK : n;
  const bool mine = k < dim;
  const int kq = mine ? k >> 2 : 0, kj = k & 3;
  const float *tiles = cb.tiles;
  double acc[RT];
#pragma unroll
  for (int i = 0; i < RT; i++) acc[i] = 0.0;

  for (int64_t base = s0; base < s1; base += B) {
    const int cnt = static_cast<int>(s1 - base < B ? s1 - base : B);
    {
      const int b = tid / RT, i = tid % RT;
      const int r = r0 + i;
      if (b < cnt) {
        const int64_t s = base + b;
        const uint32_t ip = win[s], im = win[n + s];
        const bool ok = ip < n_units && im < n_units;
        double A = 0.0, C = 0.0;
        int64_t rp = 0, rm = 0;
        if (ok) {
          rp = row_of_unit(cb, ip);
          rm = row_of_unit(cb, im);
          if (r < m) {
            const double y = static_cast<double>(xt[gmlvq_tile_at(s, r, pv.d4, GLVQ_S)]);
            const double up = y - static_cast<double>(pv.tiles[gmlvq_tile_at(rp, r, pv.d4, WAVE)]);
            const double um = y - static_cast<double>(pv.tiles[gmlvq_tile_at(rm, r, pv.d4, WAVE)]);
            A = xi[s] * up;
            C = xi[n + s] * um;
          }
        }
        s_a[b][i] = A;
        s_c[b][i] = C;
        if (i == 0) {
          s_row[b] = (first + s) % n_rows;
          s_wp[b] = ((rp >> 6) * cb.d4 * WAVE + (rp & 63)) * 4;         // the row's float offset within its group's first chunk
          s_wm[b] = ((rm >> 6) * cb.d4 * WAVE + (rm & 63)) * 4;
          s_ok[b] = ok;
        }
      }
    }
    __syncthreads();
    if (mine) {
      for (int b0 = 0; b0 < cnt; b0 += AHEAD) {
        float x[AHEAD], wp[AHEAD], wm[AHEAD];
#pragma unroll
        for (int a = 0; a < AHEAD; a++) {
          const int b = b0 + a < cnt ? b0 + a : cnt - 1;
          x[a] = rows[s_row[b] * dim + k];
          wp[a] = tiles[s_wp[b] + static_cast<int64_t>(kq) * (WAVE * 4) + kj];
          wm[a] = tiles[s_wm[b] + static_cast<int64_t>(kq) * (WAVE * 4) + kj];
        }
#pragma unroll
        for (int a = 0; a < AHEAD; a++) {
          const int b = b0 + a;
          if (b >= cnt || !s_ok[b]) continue;
          const double xd = static_cast<double>(x[a]);
          const double tp = xd - static_cast<double>(wp[a]);
          const double tm = xd - static_cast<double>(wm[a]);
#pragma unroll
          for (int i = 0; i < RT; i++) {
            const double p = s_a[b][i] * tp;
            acc[i] = acc[i] + p;
            const double q = s_c[b][i] * tm;
            acc[i] = acc[i] - q;
          }
        }
      }
    }
    __syncthreads();                                // the batch's coefficients are read
  }
  if (!mine) return;
#pragma unroll
  for (int i = 0; i < RT; i++)
    if (r0 + i < m) part[(static_cast<int64_t>(blockIdx.z) * m + (r0 + i)) * dim + k] = acc[i];
}

// Gm[e], e < len = m * dim: one chain of fp64 additions from +0.0 over the blocks in order of part[block][e], AHEAD of
// them requested ahead.
template <int AHEAD>
__global__ __launch_bounds__(GMLVQ_THREADS) void k_gmlvq_omega_reduce(const double *__restrict__ part, int64_t nblocks, int64_t len,
                                                                      double *__restrict__ Gm) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * GMLVQ_THREADS + threadIdx.x;
  if (e >= len) return;
  const double *p = part + e;
  double acc = 0.0;
  int64_t z = 0;
  for (; nblocks - z >= AHEAD; z += AHEAD) {
    double v[AHEAD];
#pragma unroll
    for (int a = 0; a < AHEAD; a++) v[a] = p[(z + a) * len];
#pragma unroll
    for (int a = 0; a < AHEAD; a++) acc = acc + v[a];
  }
  for (; z < nblocks; z++) acc = acc + p[z * len];
  Gm[e] = acc;
}

// Step 6, in place over the storage tiles: one workgroup per storage row j.  With W = (double)w_j[k]:
//   g[k]  = (Sp[j][k] - sp[j] * W) - (Sm[j][k] - sm[j] * W)                       (K9's g, into gbuf[j][.])
//   P[r]  = the chain over k in order from +0.0 of acc + g[k] * (double)omega[r][k]   (thread = r; omT is omega transposed,
//           [dim][m], so a wave reads contiguous floats; into pbuf[j][.])
//   Dl[k] = the chain over r in order from +0.0 of acc + P[r] * (double)omega[r][k]   (thread = k; om is [m][dim])
//   w_j[k] = (float)(W + a * Dl[k])
// every product rounded before it is added.  A row no sample chose in either role keeps its bits; so does the padding.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_gmlvq_update(CbView cb, const double *__restrict__ S, const uint32_t *__restrict__ hits,
                                                          const float *__restrict__ om, const float *__restrict__ omT, int m,
                                                          double *__restrict__ gbuf, double *__restrict__ pbuf, double a) {
  const int64_t row = blockIdx.x;
  if (row >= cb.n) return;
  const uint32_t u = unit_of_row(cb, row);
  const uint32_t n_units = static_cast<uint32_t>(cb.n);
  if (hits[u] == 0 && hits[n_units + u] == 0) return;
  const int dim = cb.d;
  const int64_t ld = dim + 1;
  const double *Sp = S + static_cast<int64_t>(u) * ld, *Sm = S + (static_cast<int64_t>(n_units) + u) * ld;
  const double sp = Sp[dim], sm = Sm[dim];
  float *tile = cb.tiles + ((row >> 6) * cb.d4 * WAVE + (row & 63)) * 4;
  double *g = gbuf + row * dim, *P = pbuf + row * m;
  const int tid = threadIdx.x;
  for (int k = tid; k < dim; k += THREADS) {
    const double W = static_cast<double>(tile[static_cast<int64_t>(k >> 2) * (WAVE * 4) + (k & 3)]);
    g[k] = glvq_step_g(Sp[k], Sm[k], sp, sm, W);
  }
  __syncthreads();
  for (int r = tid; r < m; r += THREADS) {
    double acc = 0.0;
    for (int k = 0; k < dim; k++) {
      const double p = g[k] * static_cast<double>(omT[static_cast<int64_t>(k) * m + r]);
      acc = acc + p;
    }
    P[r] = acc;
  }
  __syncthreads();
  for (int k = tid; k < dim; k += THREADS) {
    double acc = 0.0;
    for (int r = 0; r < m; r++) {
      const double p = P[r] * static_cast<double>(om[static_cast<int64_t>(r) * dim + k]);
      acc = acc + p;
    }
    float *w = tile + static_cast<int64_t>(k >> 2) * (WAVE * 4) + (k & 3);
    const double W = static_cast<double>(*w);
    const double step = a * acc;
    *w = static_cast<float>(W + step);
  }
}

}  // namespace somhip
