// kernels/mapset.hpp -- K7: many small maps of one shape, each resident in one workgroup's LDS
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "som_online.hpp"

namespace somhip {

// =====================================================================================
// K7: the reference's strictly online som_training (som_rout.c:600-662) for a SET of maps that share shape, data and
// schedule (vfind's trials).  K3 is one launch per iteration, and on a 12x8x5 map that launch is one workgroup and the
// time is the launch-to-launch floor; here a workgroup keeps ITS map in LDS for a whole chunk of iterations, so the
// chunk costs one launch whatever the number of maps.
//   LDS image: component-major, img[i * npad + u] -- unit u belongs to thread u % nt, so a wave reads consecutive words.
//   A thread only ever reads and writes its own units: update(t) and distance(t + 1) need no barrier between them.  The
//   one workgroup-wide step of an iteration is the winner: a DPP minimum per wave, one LDS exchange (two slots in turn,
//   so one barrier per iteration is enough); a single-wave workgroup has no barrier at all.
//   The sample of iteration t + 1 (and its mask) is fetched into registers while t computes and put into one of three
//   LDS slots before t's barrier: its readers come after that barrier, the slot's previous readers (iteration t - 2) were
//   done before the barrier of t - 1.
// The arithmetic is K3's: sq_acc over the sample's unmasked components in order, make_key(dist, unit) with the lowest
// unit winning ties and FLT_MAX to beat, lattice_sq from the winner's or the fixed point's coordinates, adapt1.
// =====================================================================================
struct MapsetShape {
  int n, d;        // units per map, components
  int npad;        // units rounded up to a wave: the image's row length
  int upt;         // units per thread: unit u = tid + k * blockDim.x, k < upt
  int dpad;        // d rounded up to 4: length of a sample slot
  int xdim, topol;
};
constexpr int MAPSET_MAX_WAVES = 16;
constexpr int MAPSET_PF = 8;                       // sample words a thread stages (d <= 8 * threads: host plan)
constexpr int MAPSET_RED_BYTES = 2 * MAPSET_MAX_WAVES * 8;
constexpr int MAPSET_LDS_LIMIT = 150 * 1024;       // dynamic LDS the kernels may ask for: a 128 KiB image, 7.5 KiB of sample slots

// the LDS of both kernels: [exchange slots][image][three sample slots][three mask slots]
struct MapsetLds {
  uint64_t *red; float *img, *xs; uint8_t *ms;
  __device__ __forceinline__ MapsetLds(unsigned char *base, const MapsetShape &s) {
    red = reinterpret_cast<uint64_t *>(base);
    img = reinterpret_cast<float *>(base + MAPSET_RED_BYTES);
    xs = img + static_cast<size_t>(s.d) * s.npad;
    ms = reinterpret_cast<uint8_t *>(xs + 3 * s.dpad);
  }
};

__device__ __forceinline__ void mapset_load(const MapsetShape &s, const float *__restrict__ g, float *img) {
  const int total = s.n * s.d;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int u = idx / s.d, i = idx - u * s.d;
    img[i * s.npad + u] = g[idx];
  }
}
__device__ __forceinline__ void mapset_store(const MapsetShape &s, const float *img, float *__restrict__ g) {
  const int total = s.n * s.d;
  for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
    const int u = idx / s.d, i = idx - u * s.d;
    g[idx] = img[i * s.npad + u];
  }
}

// a sample row on its way from global memory to an LDS slot
template <bool MASKED>
struct MapsetFetch {
  float x[MAPSET_PF];
  uint8_t m[MAPSET_PF];
  __device__ __forceinline__ void load(const MapsetShape &s, const float *__restrict__ rows, const uint8_t *__restrict__ mask, int64_t row) {
    const float *xr = rows + row * s.d;
    const uint8_t *mr = MASKED ? mask + row * s.d : nullptr;
#pragma unroll
    for (int k = 0; k < MAPSET_PF; k++) {
      const int i = threadIdx.x + k * blockDim.x;
      if (i < s.d) { x[k] = xr[i]; if (MASKED) m[k] = mr[i]; }
    }
  }
  __device__ __forceinline__ void put(const MapsetShape &s, float *xs, uint8_t *ms) const {
#pragma unroll
    for (int k = 0; k < MAPSET_PF; k++) {
      const int i = threadIdx.x + k * blockDim.x;
      if (i < s.d) { xs[i] = x[k]; if (MASKED) ms[i] = m[k]; }
    }
  }
};

// what stands between a slot's writers and its readers: the workgroup's barrier, or -- one wave, whose LDS operations
// complete in order -- only the compiler's
__device__ __forceinline__ void mapset_meet(bool one_wave) {
  if (one_wave) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
  else __syncthreads();
}

// the smallest key of this thread's units against the sample in (xs, ms)
template <bool MASKED>
__device__ __forceinline__ uint64_t mapset_thread_key(const MapsetShape &s, const float *img, const float *xs, const uint8_t *ms) {
  uint64_t best = KEY_NONE;
  for (int k = 0; k < s.upt; k++) {
    const int u = threadIdx.x + k * blockDim.x;
    if (u >= s.n) break;
    const float *c = img + u;
    float acc = 0.0f;
    for (int i = 0; i < s.d; i++) {
      if (MASKED) { if (ms[i] == 0) acc = sq_acc(acc, c[i * s.npad], xs[i]); }
      else acc = sq_acc(acc, c[i * s.npad], xs[i]);
    }
    const uint64_t key = make_key(acc, static_cast<uint32_t>(u));
    best = key < best ? key : best;
  }
  return best;
}
// ... of the workgroup: every thread returns it.  `slot`: this iteration's exchange slots; the barrier in here is the
// iteration's only one (before_meet runs ahead of it in every thread)
template <class F>
__device__ __forceinline__ uint64_t mapset_group_min(uint64_t k, uint64_t *slot, bool one_wave, F before_meet) {
  k = wave_min_u64_dpp(k);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (!one_wave && lane == 0) slot[wave] = k;
  before_meet();
  mapset_meet(one_wave);
  if (one_wave) return k;
  return wave_min_u64_dpp(lane < nw ? slot[lane] : KEY_NONE);
}

template <bool GAUSS, bool MASKED>
__global__ __launch_bounds__(1024) void k_mapset_train(MapsetShape s, float *__restrict__ maps, const float *__restrict__ rows,
                                                       const uint8_t *__restrict__ mask, const StepScalars *__restrict__ sc,
                                                       const int64_t *__restrict__ rowidx, int c, uint64_t *__restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mapset_lds[];
  const MapsetLds L(mapset_lds, s);
  const bool one_wave = blockDim.x <= WAVE;
  float *gmap = maps + static_cast<size_t>(blockIdx.x) * s.n * s.d;
  mapset_load(s, gmap, L.img);
  MapsetFetch<MASKED> f;
  f.load(s, rows, mask, rowidx[0]);
  f.put(s, L.xs, L.ms);
  mapset_meet(one_wave);

  const uint32_t xd = static_cast<uint32_t>(s.xdim);
  const int tx0 = static_cast<int>(threadIdx.x % xd), ty0 = static_cast<int>(threadIdx.x / xd);   // unit tid's coordinates
  StepScalars s_next = sc[0];
  int64_t r_next = rowidx[c > 1 ? 1 : 0];
  int cur = 0;                                     // the slot that holds iteration t's sample
  for (int t = 0; t < c; t++) {
    const StepScalars st = s_next;
    const int nxt = cur == 2 ? 0 : cur + 1;
    const float *xs = L.xs + cur * s.dpad;
    const uint8_t *ms = L.ms + cur * s.dpad;
    // iteration t + 1's scalars and sample, t + 2's row index: in flight while t computes (clamped at the chunk's end)
    const int t1 = t + 1 < c ? t + 1 : c - 1, t2 = t + 2 < c ? t + 2 : c - 1;
    s_next = sc[t1];
    f.load(s, rows, mask, r_next);
    r_next = rowidx[t2];

    const bool act = st.reach >= 0;                // (a fixed point gives a masked-out sample its reach back: som_scalars)
    const bool search = act && st.fixed < 0;
    uint64_t win = KEY_NONE;
    auto stage = [&]() { f.put(s, L.xs + nxt * s.dpad, L.ms + nxt * s.dpad); };
    if (search) {
      win = mapset_group_min(mapset_thread_key<MASKED>(s, L.img, xs, ms), L.red + (t & 1) * MAPSET_MAX_WAVES, one_wave, stage);
    } else {
      stage();
      mapset_meet(one_wave);
    }
    if (keys && threadIdx.x == 0) keys[static_cast<size_t>(blockIdx.x) * c + t] = win;

    int bx = -1, by = -1;
    if (act) {
      if (st.fixed >= 0) { bx = fixed_x(st.fixed); by = fixed_y(st.fixed); }
      else if (static_cast<uint32_t>(win >> 32) < FLT_MAX_BITS) {
        const uint32_t widx = static_cast<uint32_t>(win);
        bx = static_cast<int>(widx % xd); by = static_cast<int>(widx / xd);
      }
    }
    if (bx >= 0) {
      double den = 0.0, rcp = 0.0;
      if (GAUSS) gauss_rate_den(st.thresh, &den, &rcp);
      for (int k = 0; k < s.upt; k++) {
        const int u = threadIdx.x + k * blockDim.x;
        if (u >= s.n) break;
        int tx = tx0, ty = ty0;
        if (k > 0) { tx = static_cast<int>(static_cast<uint32_t>(u) % xd); ty = static_cast<int>(static_cast<uint32_t>(u) / xd); }
        const float lsq = lattice_sq(s.topol, bx, by, tx, ty);
        float a = st.alpha;
        if (GAUSS) {
          float h;
          if (gauss_rate_fast(lsq, den, rcp, &h)) a = st.alpha * h;
          else a = gaussian_alpha_call(lsq, st.thresh, st.alpha);
        } else if (!(lsq <= st.thresh)) continue;
        float *cu = L.img + u;
        for (int i = 0; i < s.d; i++) {
          if (MASKED) { if (ms[i] == 0) cu[i * s.npad] = adapt1(cu[i * s.npad], xs[i], a); }
          else cu[i * s.npad] = adapt1(cu[i * s.npad], xs[i], a);
        }
      }
    }
    cur = nxt;
  }
  mapset_meet(one_wave);
  mapset_store(s, L.img, gmap);
}

// find_winner_euc (lvq_pak.c:37-89) of every map of a set over data rows first + [s0, s0 + per) of the run, s0 =
// blockIdx.y * per: grid (map, sample chunk), the map in LDS as above, the same distance and the same reduction.
// keys[map][sample of the run]; the host decodes them (a sample with every component masked: there)
template <bool MASKED>
__global__ __launch_bounds__(1024) void k_mapset_winners(MapsetShape s, const float *__restrict__ maps, const float *__restrict__ rows,
                                                         const uint8_t *__restrict__ mask, int64_t n_rows, int64_t first, int64_t count,
                                                         int per, uint64_t *__restrict__ keys) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mapset_lds[];
  const MapsetLds L(mapset_lds, s);
  const bool one_wave = blockDim.x <= WAVE;
  const int64_t s0 = static_cast<int64_t>(blockIdx.y) * per;
  if (s0 >= count) return;
  const int c = static_cast<int>(count - s0 < per ? count - s0 : per);
  mapset_load(s, maps + static_cast<size_t>(blockIdx.x) * s.n * s.d, L.img);
  MapsetFetch<MASKED> f;
  f.load(s, rows, mask, (first + s0) % n_rows);
  f.put(s, L.xs, L.ms);
  mapset_meet(one_wave);
  int cur = 0;
  for (int t = 0; t < c; t++) {
    const int nxt = cur == 2 ? 0 : cur + 1;
    const int t1 = t + 1 < c ? t + 1 : c - 1;
    f.load(s, rows, mask, (first + s0 + t1) % n_rows);
    const uint64_t win = mapset_group_min(mapset_thread_key<MASKED>(s, L.img, L.xs + cur * s.dpad, L.ms + cur * s.dpad),
                                          L.red + (t & 1) * MAPSET_MAX_WAVES, one_wave,
                                          [&]() { f.put(s, L.xs + nxt * s.dpad, L.ms + nxt * s.dpad); });
    if (threadIdx.x == 0) keys[static_cast<size_t>(blockIdx.x) * count + s0 + t] = win;
    cur = nxt;
  }
}

}  // namespace somhip
