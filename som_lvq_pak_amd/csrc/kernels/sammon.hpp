// kernels/sammon.hpp -- Sammon mapping of a codebook (SOM_PAK sammon.c:130-245), bit for bit
// (part of kernels.hpp; see the notes at the top of that file)
//
// One sweep of the reference is a Jacobi step: every new (xu[j], yu[j]) is computed from the old x[], y[] only, so all
// j are independent.  What stays serial is the order of the four running sums over k inside one j.  C's promotion rules
// decide the bits (sammon.c:193-211; float = fp32, every operation rounded on its own, no contraction):
//
//   xd = x[j] - x[k]; yd = y[j] - y[k]                                float
//   dpj = (float) sqrt((double)xd * (double)xd + (double)(float)(yd * yd))      -- not symmetric in x and y
//   dt = dd(j, k); dq = dt - dpj; dr = dt * dpj                       float
//   e1x = (float)(e1x + (float)((float)(xd * dq) / dr))               float chain; e1y with yd
//   t   = (double)dq - ((double)(float)(xd * xd) * (1.0 + (double)(float)(dq / dpj))) / (double)dpj
//   e2x = (float)((double)e2x + t / (double)dr)                       double term, float running sum; e2y with yd
//   xu[j] = (float)((double)x[j] + (0.2 * (double)e1x) / fabs((double)e2x))
//   xx = float sum of xu[0..noc-1] in order; xx = xx / (float)noc; x[j] = xu[j] - xx
//
// fp32 and fp64 division and square root are the correctly rounded ones at this library's build flags.
// The four sums start at +0.0 and a sum that starts there can never become -0.0, so adding a +0.0 term is exact: the
// kernels add +0.0 where the reference skips k == j.
#pragma once
#include "common.hpp"

namespace somhip {

// =====================================================================================
// K-sammon-dist: dd(j, k) of all pairs of rows (vector_dist_euc, lvq_pak.c:291-316, no masks): the fp32 sum of
// (a_i - b_i)^2 in the order of i, three roundings per component, then (float) sqrt((double) sum).
// rows[noc][d] row-major in unit order.  A workgroup owns a 64 x 64 tile of pairs, stages 32 components of both row
// blocks in LDS and every thread owns 4 x 4 whole pairs, so the order in i is kept.  Only tiles on or above the
// diagonal are computed; (a - b)^2 == (b - a)^2 exactly, so the mirror image is a copy.
//   D      null or the full symmetric table D[k * ld + j] (the sweep reads 16 consecutive j of one k per 16 lanes)
//   pairs  null or room for `cap` pairs {j, k}, j < k, with dd == 0, in no order; *n_zero counts all of them
// =====================================================================================
constexpr int SAMMON_TILE = 64, SAMMON_DCHUNK = 32;

__global__ __launch_bounds__(256) void k_sammon_dist(const float *__restrict__ rows, int noc, int d, float *__restrict__ D,
                                                     int64_t ld, uint32_t *__restrict__ pairs, unsigned long long cap,
                                                     unsigned long long *__restrict__ n_zero) {
  if (blockIdx.x > blockIdx.y) return;
  __shared__ float sa[SAMMON_DCHUNK][SAMMON_TILE + 1], sb[SAMMON_DCHUNK][SAMMON_TILE + 1];
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int j0 = blockIdx.x * SAMMON_TILE, k0 = blockIdx.y * SAMMON_TILE;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int b = 0; b < 4; b++) acc[a][b] = 0.0f;
  for (int c0 = 0; c0 < d; c0 += SAMMON_DCHUNK) {
#pragma unroll
    for (int t = 0; t < SAMMON_TILE * SAMMON_DCHUNK / 256; t++) {
      const int idx = tid + 256 * t, i = idx & (SAMMON_DCHUNK - 1), r = idx / SAMMON_DCHUNK;
      const bool in_i = c0 + i < d;
      sa[i][r] = (in_i && j0 + r < noc) ? rows[static_cast<int64_t>(j0 + r) * d + c0 + i] : 0.0f;
      sb[i][r] = (in_i && k0 + r < noc) ? rows[static_cast<int64_t>(k0 + r) * d + c0 + i] : 0.0f;
    }
    __syncthreads();
    // components past d are 0 - 0: adding their +0.0 square to a sum that is >= +0.0 is exact
#pragma unroll 8
    for (int i = 0; i < SAMMON_DCHUNK; i++) {
      float va[4], vb[4];
#pragma unroll
      for (int a = 0; a < 4; a++) { va[a] = sa[i][tx + 16 * a]; vb[a] = sb[i][ty + 16 * a]; }
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = sq_acc(acc[a][b], va[a], vb[b]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int b = 0; b < 4; b++)
#pragma unroll
    for (int a = 0; a < 4; a++) {
      const int j = j0 + tx + 16 * a, k = k0 + ty + 16 * b;
      if (j >= noc || k >= noc) continue;
      const float dist = static_cast<float>(sqrt(static_cast<double>(acc[a][b])));
      if (D) {
        D[static_cast<int64_t>(k) * ld + j] = dist;
        if (blockIdx.x != blockIdx.y) D[static_cast<int64_t>(j) * ld + k] = dist;
      }
      if (dist == 0.0f && j < k) {
        const unsigned long long at = atomicAdd(n_zero, 1ull);
        if (pairs && at < cap) { pairs[2 * at] = static_cast<uint32_t>(j); pairs[2 * at + 1] = static_cast<uint32_t>(k); }
      }
    }
}

// the four terms of one (j, k), as the table at the top of this file spells them
struct SammonTerms { float a1x, a1y; double b2x, b2y; };
__device__ __forceinline__ SammonTerms sammon_terms(float xj, float yj, float xk, float yk, float dt) {
  const float xd = xj - xk, yd = yj - yk;
  const float ysq = yd * yd;
  const double xsq_d = static_cast<double>(xd) * static_cast<double>(xd);
  const float dpj = static_cast<float>(sqrt(xsq_d + static_cast<double>(ysq)));
  const float dq = dt - dpj, dr = dt * dpj;
  const float xq = xd * dq, yq = yd * dq;
  const float quot = dq / dpj;
  const double fac = 1.0 + static_cast<double>(quot);
  const double dpd = static_cast<double>(dpj), drd = static_cast<double>(dr), dqd = static_cast<double>(dq);
  const float xsq = xd * xd;
  const double px = static_cast<double>(xsq) * fac, py = static_cast<double>(ysq) * fac;
  const double tx = dqd - px / dpd, ty = dqd - py / dpd;
  SammonTerms t;
  t.a1x = xq / dr;
  t.a1y = yq / dr;
  t.b2x = tx / drd;
  t.b2y = ty / drd;
  return t;
}
__device__ __forceinline__ float sammon_correct(float xj, float e1, float e2) {   // sammon.c:210-211, MAGIC = 0.2
  const double step = 0.2 * static_cast<double>(e1);
  return static_cast<float>(static_cast<double>(xj) + step / fabs(static_cast<double>(e2)));
}

// =====================================================================================
// K-sammon-sweep: xu[], yu[] of one iteration.  The square root and the seven divisions of a pair are independent of
// every other pair, only the sums are ordered, so term evaluation is split from accumulation.  A workgroup owns 16
// values of j and walks k in chunks of 64: its 256 threads compute the terms of the chunk's 1024 pairs and park them in
// LDS; then 16 lanes of wave w add chain w (e1x, e1y, e2x, e2y) of their j in the order of k.  noc / 16 workgroups.
// (A form with lane = j and a serial loop over k in each lane, noc / 64 waves, was 1.8 to 10 times slower at every
// size measured: profiles/sammon_sweep.txt.)
// =====================================================================================
constexpr int SAMMON_JB = 16, SAMMON_KC = 64;

__global__ __launch_bounds__(256) void k_sammon_sweep(const float *__restrict__ D, int64_t ld, int noc,
                                                      const float *__restrict__ x, const float *__restrict__ y,
                                                      float *__restrict__ xu, float *__restrict__ yu) {
  __shared__ float s1x[SAMMON_KC][SAMMON_JB], s1y[SAMMON_KC][SAMMON_JB];
  __shared__ double s2x[SAMMON_KC][SAMMON_JB], s2y[SAMMON_KC][SAMMON_JB];
  __shared__ float fin[4][SAMMON_JB];
  const int tid = threadIdx.x, jl = tid & (SAMMON_JB - 1), kq = tid / SAMMON_JB;
  const int wave = tid >> 6, lane = tid & 63;
  const int j0 = blockIdx.x * SAMMON_JB, j = j0 + jl;
  const int jj = j < noc ? j : noc - 1;
  const float xj = x[jj], yj = y[jj];
  const float *col = D + jj;
  float chain = 0.0f;
  for (int k0 = 0; k0 < noc; k0 += SAMMON_KC) {
#pragma unroll
    for (int p = 0; p < SAMMON_KC * SAMMON_JB / 256; p++) {
      const int kl = kq + (256 / SAMMON_JB) * p, k = k0 + kl;
      const int kk = k < noc ? k : noc - 1;
      const SammonTerms t = sammon_terms(xj, yj, x[kk], y[kk], col[static_cast<int64_t>(kk) * ld]);
      const bool on = k < noc && k != jj;
      s1x[kl][jl] = on ? t.a1x : 0.0f;
      s1y[kl][jl] = on ? t.a1y : 0.0f;
      s2x[kl][jl] = on ? t.b2x : 0.0;
      s2y[kl][jl] = on ? t.b2y : 0.0;
    }
    __syncthreads();
    if (lane < SAMMON_JB) {
      if (wave < 2) {
        const float(*s)[SAMMON_JB] = wave == 0 ? s1x : s1y;
#pragma unroll 8
        for (int kl = 0; kl < SAMMON_KC; kl++) chain = chain + s[kl][lane];
      } else {
        const double(*s)[SAMMON_JB] = wave == 2 ? s2x : s2y;
#pragma unroll 8
        for (int kl = 0; kl < SAMMON_KC; kl++) chain = static_cast<float>(static_cast<double>(chain) + s[kl][lane]);
      }
    }
    __syncthreads();
  }
  if (lane < SAMMON_JB) fin[wave][lane] = chain;
  __syncthreads();
  if (tid < SAMMON_JB && j < noc) {
    xu[j] = sammon_correct(xj, fin[0][tid], fin[2][tid]);
    yu[j] = sammon_correct(yj, fin[1][tid], fin[3][tid]);
  }
}

// =====================================================================================
// K-sammon-centre: the centre of mass (sammon.c:215-225).  The float sums over xu[] and yu[] are ordered, so one lane
// each adds them (staged through LDS by the whole workgroup); then x = xu - xx, y = yu - yy.  One workgroup.
// =====================================================================================
constexpr int SAMMON_CENTRE_CHUNK = 2048;

__global__ __launch_bounds__(256) void k_sammon_centre(const float *__restrict__ xu, const float *__restrict__ yu,
                                                       float *__restrict__ x, float *__restrict__ y, int noc) {
  __shared__ float bx[SAMMON_CENTRE_CHUNK], by[SAMMON_CENTRE_CHUNK];
  __shared__ float mean[2];
  const int tid = threadIdx.x;
  float sum = 0.0f;
  for (int c0 = 0; c0 < noc; c0 += SAMMON_CENTRE_CHUNK) {
    const int cnt = noc - c0 < SAMMON_CENTRE_CHUNK ? noc - c0 : SAMMON_CENTRE_CHUNK;
    for (int t = tid; t < cnt; t += 256) { bx[t] = xu[c0 + t]; by[t] = yu[c0 + t]; }
    __syncthreads();
    if (tid == 0 || tid == 64) {                          // lane 0 of two waves: one chain each
      const float *b = tid == 0 ? bx : by;
#pragma unroll 8
      for (int t = 0; t < cnt; t++) sum = sum + b[t];
    }
    __syncthreads();
  }
  if (tid == 0) mean[0] = sum / static_cast<float>(noc);
  if (tid == 64) mean[1] = sum / static_cast<float>(noc);
  __syncthreads();
  const float xx = mean[0], yy = mean[1];
  for (int i = tid; i < noc; i += 256) { x[i] = xu[i] - xx; y[i] = yu[i] - yy; }
}

// =====================================================================================
// K-sammon-error: the mapping error's two sums (sammon.c:227-240): per pair the reference's float term ee * ee / d and d,
// summed in double by a tree.  The reference adds them one after the other in fp32, which no parallel sum reproduces:
// this number (printed with %7.3f from -v 2 up) is close to the reference's, not bit-equal; nothing is computed from it.
// part[2 * block] = sum of the terms, part[2 * block + 1] = sum of the distances; the host adds the blocks.
// =====================================================================================
__global__ __launch_bounds__(256) void k_sammon_error(const float *__restrict__ D, int64_t ld, int noc,
                                                      const float *__restrict__ x, const float *__restrict__ y,
                                                      double *__restrict__ part) {
  __shared__ double se[256], st[256];
  const int tid = threadIdx.x;
  double e = 0.0, tot = 0.0;
  for (int j = 1 + blockIdx.x; j < noc; j += gridDim.x) {
    const float xj = x[j], yj = y[j];
    for (int k = tid; k < j; k += 256) {
      const float dist = D[static_cast<int64_t>(j) * ld + k];
      const float xd = xj - x[k], yd = yj - y[k];
      const float ysq = yd * yd;
      const double xsq_d = static_cast<double>(xd) * static_cast<double>(xd);
      const float ee = dist - static_cast<float>(sqrt(xsq_d + static_cast<double>(ysq)));
      const float sq = ee * ee;
      e += static_cast<double>(sq / dist);
      tot += static_cast<double>(dist);
    }
  }
  se[tid] = e; st[tid] = tot;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if (tid < s) { se[tid] += se[tid + s]; st[tid] += st[tid + s]; }
    __syncthreads();
  }
  if (tid == 0) { part[2 * blockIdx.x] = se[0]; part[2 * blockIdx.x + 1] = st[0]; }
}

}  // namespace somhip
