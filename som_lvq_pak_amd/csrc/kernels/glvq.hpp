// kernels/glvq.hpp -- K9: batch GLVQ -- the class-wise exact winner search, the per-sample terms, the per-prototype
// ordered fp64 sums of both roles, and the update
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "batchmap.hpp"

namespace somhip {

// =====================================================================================
// K9: one epoch of batch GLVQ (the definition is in include/somhip.h).
//
//   search   keys2[s][2]: the key (distance bits, row) of the nearest row of the sample's own class ([0]) and of the
//            nearest row of any other class ([1]).  Direct route: k_scan_class over every row.  List route: the exact
//            top-8 lists of the engine's k-NN search, k_glvq_pick takes each role's first entry; the samples whose list
//            lacks a role are listed and go through k_scan_class alone.
//   terms    k_glvq_terms: xi+, xi-, f per sample in fp64, the two winners, their counts and the correct count by
//            integer atomics; then K8's k_batchmap_starts and the stable sort by winner, once per role.
//   sums     k_glvq_sums: per (prototype, role) one chain of fp64 additions from +0.0 over the role's list in data order
//            of xi * (double)x[k]; the trailing column carries the sum of xi, and for role + the sum of f goes to cost[].
//            k_glvq_sums<true> continues the chains a piece of the data left in S and cost (somhip_glvq_accumulate), and
//            k_glvq_counts behind it adds the piece's counts to the state's integers.
//   update   k_glvq_update: w <- (float)(W + a * ((Sp - sp W) - (Sm - sm W))) over the storage tiles, in place.
//
// Bodies stated here once and used by K11 and K12 too: glvq_sums_chain (k_glvq_sums, k_grlvq_sums), glvq_step_g (the g of
// a chosen row: k_glvq_update, k_grlvq_update, k_gmlvq_update) and glvq_update_tiles (k_glvq_update, k_grlvq_update).  The
// search is not among them: k_scan_class and K11's k_scan_class_weighted are written out each, since one body behind a
// function boundary changed their register allotment (profiles/kernel_bodies_vs_parent.txt).
//
// No floating-point atomics anywhere: every sum is a function of the data, the codebook and the shape alone.
// =====================================================================================
constexpr int GLVQ_S = 32;                    // samples of a search tile (K1's SCAN_S)
constexpr int GLVQ_R = 4;                     // row groups per wave of the search on codebooks of 16 groups and more
constexpr int GLVQ_THREADS = 256;             // the per-sample passes
constexpr int GLVQ_SUM_AHEAD = 8;             // list entries requested ahead of the chain

// The sample tiles of the listed samples sel[0 .. count) of a run (run sample s is data row (first + s) % n_rows), in
// k_pack_samples' layout: what the direct route reads when it runs over a remainder.
template <int S>
__global__ __launch_bounds__(256) void k_glvq_pack_listed(const float *__restrict__ rows, int64_t n_rows, int d, int d4, int64_t first,
                                                          const uint32_t *__restrict__ sel, int64_t count,
                                                          float4 *__restrict__ xt) {
  const int64_t sb = blockIdx.x;
  for (int e = threadIdx.x; e < d4 * S; e += blockDim.x) {
    const int q = e / S, s = e % S;
    const int64_t j = sb * S + s;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < count) {
      const int64_t r = (first + static_cast<int64_t>(sel[j])) % n_rows;
#pragma unroll
      for (int i = 0; i < 4; i++)
        if (q * 4 + i < d) v[i] = rows[r * d + q * 4 + i];
    }
    xt[(sb * d4 + q) * S + s] = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// The class-wise winner scan: K1's shape (kernels/scan_exact.hpp) -- lane = code row, R row groups per wave, S running
// fp32 sums per row in registers, the sample tile at a wave-uniform address, every sum formed by sq_acc in dimension
// order -- with two keys per sample out of the epilogue: the minimum over the lanes whose row carries the sample's label
// and the minimum over the lanes whose row does not.  A lane's row labels are loaded once; the tile's sample labels sit
// in LDS, read at a wave-uniform address.  Dead lanes carry KEY_NONE in both roles.  The four waves are merged through
// LDS, then one 64-bit atomicMin per (sample, role) into keys2 with the row as the tag: the lowest row wins among
// equal distances.
// Tile sample j (< count) is run sample sel[j], or base + j without a list; its label is that of data row
// (first + run sample) % n_rows and its keys are keys2[2 * run sample + role].  cb_labels is indexed by unit.
template <int S, int R>
__global__ __launch_bounds__(256) void k_scan_class(CbView cb, const float4 *__restrict__ xt, int64_t count,
                                                    const int32_t *__restrict__ cb_labels, const int32_t *__restrict__ ds_labels,
                                                    int64_t n_rows, int64_t first, int64_t base, const uint32_t *__restrict__ sel,
                                                    uint64_t *__restrict__ keys2) {
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
      smp = sel ? static_cast<int64_t>(sel[j]) : base + j;
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
#pragma unroll
      for (int s = 0; s < S; s++) {
        const float4 x = xtile[q * S + s];          // wave-uniform address
#pragma unroll
        for (int r = 0; r < R; r++) {
          float a = acc[r][s];
          a = sq_acc(a, c[r].x, x.x);
          a = sq_acc(a, c[r].y, x.y);
          a = sq_acc(a, c[r].z, x.z);
          a = sq_acc(a, c[r].w, x.w);
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

// The list route's pick.  Per sample i of a chunk (run sample off + i) from its ascending top-K list keys[i][stride]
// (SOMHIP_TIE_FIRST keys: plain row tags, so the list is ordered by (distance, row)): the first entry whose row carries
// the sample's label and the first whose row does not are those roles' exact winners.  A sample whose list lacks a role
// (or ends before it) gets KEY_NONE in both keys and is appended to rem[] through an integer counter, in any order.
__global__ __launch_bounds__(GLVQ_THREADS) void k_glvq_pick(const uint64_t *__restrict__ keys, int stride, int width, int64_t off,
                                                            int64_t count, uint32_t n_units, const int32_t *__restrict__ cb_labels,
                                                            const int32_t *__restrict__ ds_labels, int64_t n_rows, int64_t first,
                                                            uint64_t *__restrict__ keys2, uint32_t *__restrict__ rem,
                                                            uint32_t *__restrict__ rem_count) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * GLVQ_THREADS + threadIdx.x;
  if (i >= count) return;
  const int64_t smp = off + i;
  const int32_t ls = ds_labels[(first + smp) % n_rows];
  uint64_t own = KEY_NONE, other = KEY_NONE;
  for (int j = 0; j < width; j++) {
    const uint64_t k = keys[i * stride + j];
    const uint32_t u = static_cast<uint32_t>(k);
    if (static_cast<uint32_t>(k >> 32) >= FLT_MAX_BITS || u >= n_units) break;    // the list ends here
    if (cb_labels[u] == ls) { if (own == KEY_NONE) own = k; }
    else if (other == KEY_NONE) other = k;
  }
  if (own == KEY_NONE || other == KEY_NONE) {
    own = other = KEY_NONE;
    rem[atomicAdd(rem_count, 1u)] = static_cast<uint32_t>(smp);
  }
  keys2[2 * smp] = own;
  keys2[2 * smp + 1] = other;
}

// Step 3 of the definition, per sample s of the run from keys2[s][2], every operation one fp64 rounding in the order
// written: xi[0][s] = xi+, xi[1][s] = xi-, f[s]; win[0][s] / win[1][s] = the winners (n_units for a sample without both),
// idx[s] = s; hits[role][winner]++ and *correct += (key+ < key-) by integer atomics.  xi, win and hits hold role + in
// their first half (n, n, n_units entries) and role - in their second.
__global__ __launch_bounds__(GLVQ_THREADS) void k_glvq_terms(const uint64_t *__restrict__ keys2, int64_t n, uint32_t n_units, double beta,
                                                             double *__restrict__ xi, double *__restrict__ f,
                                                             uint32_t *__restrict__ win, uint32_t *__restrict__ idx,
                                                             uint32_t *__restrict__ hits, uint32_t *__restrict__ correct) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * GLVQ_THREADS + threadIdx.x;
  if (s >= n) return;
  const uint64_t kp = keys2[2 * s], km = keys2[2 * s + 1];
  const uint32_t ip = static_cast<uint32_t>(kp), im = static_cast<uint32_t>(km);
  const bool has = kp != KEY_NONE && km != KEY_NONE && ip < n_units && im < n_units;
  double xp = 0.0, xm = 0.0, fv = 0.0;
  if (has) {
    const double dp = static_cast<double>(__uint_as_float(static_cast<uint32_t>(kp >> 32)));
    const double dm = static_cast<double>(__uint_as_float(static_cast<uint32_t>(km >> 32)));
    const double D = dp + dm;
    const bool zero = D == 0.0;
    double mu = 0.0;
    if (!zero) { const double num = dp - dm; mu = num / D; }
    double fp = 1.0;
    fv = mu;
    if (beta != 0.0) {
      const double t = beta * mu;
      const double ex = exp(-t);
      const double den = 1.0 + ex;
      fv = 1.0 / den;
      const double bf = beta * fv;
      const double om = 1.0 - fv;
      fp = bf * om;
    }
    if (!zero) {
      const double four = 4.0 * fp;
      const double DD = D * D;
      const double np = four * dm, nm = four * dp;
      xp = np / DD;
      xm = nm / DD;
    }
    atomicAdd(hits + ip, 1u);
    atomicAdd(hits + n_units + im, 1u);
    if (kp < km) atomicAdd(correct, 1u);
  }
  xi[s] = xp;
  xi[n + s] = xm;
  f[s] = fv;
  win[s] = has ? ip : n_units;
  win[n + s] = has ? im : n_units;
  idx[s] = static_cast<uint32_t>(s);
}

// Step 4.  One wave per (prototype u = blockIdx.x, 64 columns, role = blockIdx.z), lane = column k.  S[role][u][k], k < d:
// the chain of fp64 additions from +0.0 of xi[role][s] * (double)x_s[k] -- a multiply, then an add -- over the role's list
// of u in data order (sample s is data row (first + s) % n_rows, first < n_rows); column k = d: the same chain over xi
// alone (xi * 1.0 is xi); column k = d + 1 of role +: the chain over f[s], written to cost[u].  S is [2][n_units][d + 1].
// The list is known, so AHEAD (GLVQ_SUM_AHEAD) entries -- sample, weight, row element -- are requested before their additions
// run.  One body, glvq_sums_chain, gives k_glvq_sums<CONT> below and k_grlvq_sums<AHEAD> (kernels/grlvq.hpp).
// CONT: the data come in pieces and S, cost hold what the pieces before this one left (all +0.0 before the first): every
// chain goes on from its stored value, and a (u, role) without a sample in this piece is left as it stands.  A chain from a
// stored +0.0 is the chain from +0.0, so the pieces leave the bits of one call over their rows in order.  A compile-time
// flag (k_batchmap_sums<true>'s way): the one-call kernels have no load of S ahead of their chains.
// RELEVANCE (K11's step 4, k_grlvq_sums in kernels/grlvq.hpp): a second accumulator in the same lane, for k < d
// R[role][u][k] = the chain of fp64 additions from +0.0 over the same list of  xi * (td * td),  td = (double)x_s[k] -
// (double)w_u[k]: a subtraction, two multiplications and an addition, each rounded.  w_u[k] is read once from the storage
// tiles of cb (null without RELEVANCE).  R is [2][n_units][d].
template <bool CONT, bool RELEVANCE, int AHEAD>
__device__ __forceinline__ void glvq_sums_chain(const CbView *cb, const float *__restrict__ rows, int64_t n_rows, int d, int64_t first,
                                                int64_t n, uint32_t n_units, const uint32_t *__restrict__ list,
                                                const uint32_t *__restrict__ starts, const double *__restrict__ xi,
                                                const double *__restrict__ f, double *__restrict__ S, double *__restrict__ R,
                                                double *__restrict__ cost) {
  const uint32_t u = blockIdx.x, role = blockIdx.z;
  const int k = static_cast<int>(blockIdx.y) * BM_SUM_DIMS + static_cast<int>(threadIdx.x);
  if (k > d + 1 || (k == d + 1 && role != 0)) return;
  const uint32_t *lst = list + static_cast<int64_t>(role) * n;
  const uint32_t *st = starts + static_cast<int64_t>(role) * (n_units + 1);
  const double *wt = k == d + 1 ? f : xi + static_cast<int64_t>(role) * n;
  const uint32_t lo = st[u], hi = st[u + 1];
  double W = 0.0;
  if constexpr (RELEVANCE) {
    if (k < d) {
      const int64_t row = row_of_unit(*cb, u);
      const float *tile = reinterpret_cast<const float *>(tile_ptr(*cb, row >> 6, k >> 2, static_cast<int>(row & 63)));
      W = static_cast<double>(tile[k & 3]);
    }
  }
  auto elem = [&](uint32_t s) -> float {
    return k >= d ? 1.0f : rows[run_row(first, s, n_rows) * d + k];
  };
  double acc = 0.0, rel = 0.0;
  auto add = [&](double ws, double xd) {
    const double p = ws * xd;
    acc += p;
    if constexpr (RELEVANCE) {
      const double td = xd - W;
      const double tt = td * td;
      const double pr = ws * tt;
      rel += pr;
    }
  };
  if (CONT) {
    if (lo == hi) return;                                     // no sample of this piece for (u, role): the chains stand
    acc = k == d + 1 ? cost[u] : S[(static_cast<int64_t>(role) * n_units + u) * (d + 1) + k];
  }
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
    for (int a = 0; a < AHEAD; a++) add(w[a], static_cast<double>(x[a]));
  }
  for (; i < hi; i++) {                                         // (the tail asks for its two loads in the order each kernel
    const uint32_t s = lst[i];                                  // had them, so both keep their instructions)
    if constexpr (RELEVANCE) { const double xd = static_cast<double>(elem(s)); add(wt[s], xd); }
    else add(wt[s], static_cast<double>(elem(s)));
  }
  if (k == d + 1) { cost[u] = acc; return; }
  S[(static_cast<int64_t>(role) * n_units + u) * (d + 1) + k] = acc;
  if constexpr (RELEVANCE)
    if (k < d) R[(static_cast<int64_t>(role) * n_units + u) * d + k] = rel;
}
template <bool CONT>
__global__ __launch_bounds__(BM_SUM_DIMS) void k_glvq_sums(const float *__restrict__ rows, int64_t n_rows, int d, int64_t first,
                                                           int64_t n, uint32_t n_units, const uint32_t *__restrict__ list,
                                                           const uint32_t *__restrict__ starts, const double *__restrict__ xi,
                                                           const double *__restrict__ f, double *__restrict__ S,
                                                           double *__restrict__ cost) {
  glvq_sums_chain<CONT, false, GLVQ_SUM_AHEAD>(nullptr, rows, n_rows, d, first, n, n_units, list, starts, xi, f, S, nullptr, cost);
}

// The integers of the state of an epoch over data in pieces (somhip_glvq_accumulate), behind a piece's k_glvq_sums<true>:
// counts[role][u] (np, nm) grow by the piece's hits[role][u], one thread per element; thread 0 also takes the piece into
// the tail: tail[0] (samples) grows by n, tail[1] (correct) by the piece's *correct.  One writer per word, no atomics.
__global__ __launch_bounds__(GLVQ_THREADS) void k_glvq_counts(const uint32_t *__restrict__ hits, const uint32_t *__restrict__ correct,
                                                              uint64_t n, uint32_t n_words, uint32_t *__restrict__ counts,
                                                              uint64_t *__restrict__ tail) {
  const uint32_t i = blockIdx.x * GLVQ_THREADS + threadIdx.x;
  if (i < n_words) counts[i] += hits[i];
  if (i == 0) { tail[0] += n; tail[1] += *correct; }
}

// The step of a chosen row j at component k, with W = (double)w_j[k]: g = (Sp[j][k] - sp[j] * W) - (Sm[j][k] - sm[j] * W),
// five roundings in the order written.  K9's, K11's and K12's updates all start from it.
__device__ __forceinline__ double glvq_step_g(double Spk, double Smk, double sp, double sm, double W) {
  const double pw = sp * W, mw = sm * W;
  const double gp = Spk - pw, gm = Smk - mw;
  return gp - gm;
}

// Step 5, in place over the storage tiles: thread = (row group, chunk of 4 dims, lane).  With W = (double)w_j[k] and g of
// glvq_step_g: w_j[k] = (float)(W + a * g), or with RELEVANCE (K11's step 6) (float)(W + (a * (double)lam[k]) * g), lam the
// float4[d4] tile of the weighted search read as floats.  A row no sample chose in either role (hits of both 0) keeps its
// bits; so does the padding.  The body of k_glvq_update and of k_grlvq_update (kernels/grlvq.hpp).
template <int THREADS, bool RELEVANCE>
__device__ __forceinline__ void glvq_update_tiles(const CbView &cb, const double *__restrict__ S, const uint32_t *__restrict__ hits,
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
    const double gg = glvq_step_g(Sp[k], Sm[k], sp, sm, W);
    double al = a;
    if constexpr (RELEVANCE) al = a * static_cast<double>(lam[k]);
    const double step = al * gg;
    v[j] = static_cast<float>(W + step);
  }
  *cp = make_float4(v[0], v[1], v[2], v[3]);
}
__global__ __launch_bounds__(GLVQ_THREADS) void k_glvq_update(CbView cb, const double *__restrict__ S, const uint32_t *__restrict__ hits,
                                                              double a) {
  glvq_update_tiles<GLVQ_THREADS, false>(cb, S, hits, nullptr, a);
}

}  // namespace somhip
