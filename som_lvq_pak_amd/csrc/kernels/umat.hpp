// kernels/umat.hpp -- the U-matrix of a map (SOM_PAK map.c:130-989), bit for bit
// (part of kernels.hpp; see the notes at the top of that file)
//
// The map is mx x my units, unit (i, j) is row j * mx + i; the matrix is ux x uy = (2 mx - 1) x (2 my - 1) floats,
// stored here as u[y * ux + x] = the reference's uvalue[x][y].  calc_umatrix fills it in four steps, each a kernel:
//
//   distances  every entry with an odd x or an odd y is the distance of two neighbouring units (map.c:138-271):
//                temp = (double)(float)(a_k - b_k); sum += temp * temp in the order of k, in double; (float) sqrt(sum)
//              The square of a widened float is exact in double, so only the float subtraction and the order of the
//              double additions decide the bits.  rect: (i+1, j) -> u[2i+1][2j], (i, j+1) -> u[2i][2j+1] and the two
//              diagonals -> u[2i+1][2j+1] = (sqrt(dz1)/sqrt(2.0) + sqrt(dz2)/sqrt(2.0))/2.  hexa: (i+1, j) as in rect;
//              the two lower neighbours of (i, j) are (i-1, j+1) and (i, j+1) on even j, (i, j+1) and (i+1, j+1) on
//              odd j, at u[2i-1][2j+1] / u[2i][2j+1] and u[2i][2j+1] / u[2i+1][2j+1].
//   units      every entry with even x and even y is the median of the distance entries around it (map.c:275-452):
//              sorted as doubles, the middle one of an odd count, (lo + hi) / 2.0 of the two middle ones of an even
//              count.  The reference's ladder of edge and corner cases lists, in every case, exactly the entries of
//              the 4-neighbourhood (rect) or of the 6-neighbourhood of that lattice row (hexa) that lie inside the matrix.
//   min / max  over all entries (map.c:474-485)
//   scale      u = (float)(1.0 - ((double)u - min) / bw), bw = max - min (map.c:493-497)
//
// average_umatrix (map.c:525-769) and median_umatrix (:771-989) run out of place over the scaled matrix.  Both read
// the same entries: outside the four corners, the entries inside the matrix of a fixed list -- rect: N, W, centre, E, S;
// hexa: the two entries above (left pair on y % 4 in {0, 3}, right pair on {1, 2}), W, centre, E, the two below (left
// pair on y % 4 in {0, 1}, right pair on {2, 3}) -- in that order, and the corners in an order of their own.  The average
// adds them as floats in the order written and divides by the count: rect by a double literal (the float sum is widened),
// hexa by a (float) constant.  A float quotient is the double quotient rounded once more (53 >= 2 * 24 + 2 bits), so
// both are taken in double here.  The median takes the upper middle element; rect's east border lists its W entry twice.
//
// fp64 division and square root are the correctly rounded ones at this library's build flags (see sammon.hpp).
#pragma once
#include "common.hpp"

namespace somhip {

constexpr int UMAT_TOPOL_RECT = 4;       // SOMHIP_TOPOL_RECT; everything else here is hexa

struct UmatDims {
  int mx, my, ux, uy, topol;
};

// The kernels are compiled in a translation unit of their own (csrc/umat.hip defines SOMHIP_UMAT_DEFINE), so the code
// object of the training kernels stays byte for byte what it is without them: in one object, the hot kernels of the SOM
// step measured 3 % slower at identical instructions (profiles/umatrix_vs_host.txt).  somhip.hip sees the declarations.
__global__ __launch_bounds__(256) void k_umat_dist(CbView cb, UmatDims m, float *__restrict__ u);
__global__ __launch_bounds__(256) void k_umat_units(UmatDims m, float *__restrict__ u);
__global__ __launch_bounds__(256) void k_umat_minmax(const float *__restrict__ u, int64_t count, uint32_t *__restrict__ mm);
__global__ __launch_bounds__(256) void k_umat_scale(float *__restrict__ u, int64_t count, double lo, double bw);
__global__ __launch_bounds__(256) void k_umat_average(UmatDims m, const float *__restrict__ u, float *__restrict__ out);
__global__ __launch_bounds__(256) void k_umat_median(UmatDims m, const float *__restrict__ u, float *__restrict__ out);

#ifdef SOMHIP_UMAT_DEFINE

// (double)(float)(a - b) squared, added to acc: the float subtraction rounds, the rest of the term is exact
__device__ __forceinline__ double umat_acc(double acc, float a, float b) {
  const float t = a - b;
  const double td = static_cast<double>(t);
  return acc + td * td;
}

// the double sum of one pair of rows over the first d components, in order
__device__ __forceinline__ double umat_pair(const CbView &cb, int64_t ra, int64_t rb) {
  const float4 *pa = tile_ptr(cb, ra >> 6, 0, static_cast<int>(ra & 63));
  const float4 *pb = tile_ptr(cb, rb >> 6, 0, static_cast<int>(rb & 63));
  double acc = 0.0;
  const int whole = cb.d >> 2;
#pragma unroll 4
  for (int q = 0; q < whole; q++) {
    const float4 a = pa[static_cast<int64_t>(q) * WAVE], b = pb[static_cast<int64_t>(q) * WAVE];
    acc = umat_acc(acc, a.x, b.x);
    acc = umat_acc(acc, a.y, b.y);
    acc = umat_acc(acc, a.z, b.z);
    acc = umat_acc(acc, a.w, b.w);
  }
  const int rest = cb.d & 3;
  if (rest) {
    const float4 a = pa[static_cast<int64_t>(whole) * WAVE], b = pb[static_cast<int64_t>(whole) * WAVE];
    acc = umat_acc(acc, a.x, b.x);
    if (rest > 1) acc = umat_acc(acc, a.y, b.y);
    if (rest > 2) acc = umat_acc(acc, a.z, b.z);
  }
  return acc;
}

// =====================================================================================
// K-umat-dist: one lane = one storage row (so the lane's own float4 loads are the coalesced 1 KiB of its row group,
// in the reference's row order and in 8x8 patch order alike), blockIdx.y = which neighbour: 0 the unit to the right,
// 1 and 2 the two below (rect: 1 = (i, j+1), 2 = both diagonals).  A pair's components are summed by one lane, in order.
// The codebook is a whole map (row_offset 0, no interleave): row_of_unit finds every neighbour.
// =====================================================================================
__global__ __launch_bounds__(256) void k_umat_dist(CbView cb, UmatDims m, float *__restrict__ u) {
  const int64_t row = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (row >= cb.n) return;
  int i, j;
  txty_of_row(cb, row, i, j);
  const int dir = blockIdx.y;
  const uint32_t mx = static_cast<uint32_t>(m.mx);
  const uint32_t unit = static_cast<uint32_t>(j) * mx + static_cast<uint32_t>(i);
  const bool right = i < m.mx - 1, below = j < m.my - 1;
  if (dir == 0) {
    if (!right) return;
    const double s = umat_pair(cb, row, row_of_unit(cb, unit + 1));
    u[static_cast<int64_t>(2 * j) * m.ux + 2 * i + 1] = static_cast<float>(sqrt(s));
    return;
  }
  if (!below) return;
  float *out = u + static_cast<int64_t>(2 * j + 1) * m.ux;
  if (m.topol == UMAT_TOPOL_RECT) {
    if (dir == 1) {
      out[2 * i] = static_cast<float>(sqrt(umat_pair(cb, row, row_of_unit(cb, unit + mx))));
    } else if (right) {
      const int64_t r_e = row_of_unit(cb, unit + 1), r_s = row_of_unit(cb, unit + mx), r_se = row_of_unit(cb, unit + mx + 1);
      const double dz1 = umat_pair(cb, row, r_se), dz2 = umat_pair(cb, r_s, r_e);
      const double root2 = sqrt(2.0);
      out[2 * i + 1] = static_cast<float>((sqrt(dz1) / root2 + sqrt(dz2) / root2) / 2);
    }
    return;
  }
  const bool odd = (j & 1) != 0;
  if (dir == 1) {                 // dy: (i, j+1) on odd j, (i-1, j+1) on even j
    if (odd) out[2 * i] = static_cast<float>(sqrt(umat_pair(cb, row, row_of_unit(cb, unit + mx))));
    else if (i > 0) out[2 * i - 1] = static_cast<float>(sqrt(umat_pair(cb, row, row_of_unit(cb, unit + mx - 1))));
  } else {                        // dz: (i, j+1) on even j, (i+1, j+1) on odd j
    if (!odd) out[2 * i] = static_cast<float>(sqrt(umat_pair(cb, row, row_of_unit(cb, unit + mx))));
    else if (right) out[2 * i + 1] = static_cast<float>(sqrt(umat_pair(cb, row, row_of_unit(cb, unit + mx + 1))));
  }
}

// ---- the entries a pass reads around (x, y) ------------------------------------------------------------------
struct UmatList {
  int n;
  float v[7];
  __device__ __forceinline__ void put(const float *__restrict__ u, const UmatDims &m, int x, int y) {
    if (x >= 0 && y >= 0 && x < m.ux && y < m.uy) v[n++] = u[static_cast<int64_t>(y) * m.ux + x];
  }
};

// the distance entries around unit position (x, y), both even (map.c:275-452)
__device__ __forceinline__ void umat_unit_list(const float *__restrict__ u, const UmatDims &m, int x, int y, UmatList &l) {
  l.n = 0;
  l.put(u, m, x - 1, y);
  l.put(u, m, x + 1, y);
  if (m.topol == UMAT_TOPOL_RECT) {
    l.put(u, m, x, y - 1);
    l.put(u, m, x, y + 1);
    return;
  }
  const int s = (y % 4) ? 0 : -1;           // lattice rows with y % 4 == 0 have their lower and upper pair to the left
  l.put(u, m, x + s, y - 1);
  l.put(u, m, x + s + 1, y - 1);
  l.put(u, m, x + s, y + 1);
  l.put(u, m, x + s + 1, y + 1);
}

// the entries average_umatrix adds at (x, y), in its order (map.c:541-738); median_umatrix reads the same ones, and
// `twice_w` lists rect's W entry a second time on the east border (map.c:810-814)
__device__ __forceinline__ void umat_filter_list(const float *__restrict__ u, const UmatDims &m, int x, int y, bool twice_w,
                                                 UmatList &l) {
  l.n = 0;
  const int xe = m.ux - 1, ye = m.uy - 1;
  const bool rect = m.topol == UMAT_TOPOL_RECT;
  if ((x == 0 || x == xe) && (y == 0 || y == ye)) {           // the corners, each in the order written
    const int ix = x == 0 ? 1 : -1, iy = y == 0 ? 1 : -1;     // towards the inside
    if (rect) {
      if (x == 0 && y == 0) { l.put(u, m, x + ix, y); l.put(u, m, x, y + iy); l.put(u, m, x, y); }
      else { l.put(u, m, x + ix, y); l.put(u, m, x, y); l.put(u, m, x, y + iy); }
    } else if (x == 0 && y == 0) { l.put(u, m, 1, 0); l.put(u, m, 0, 0); l.put(u, m, 0, 1); }
    else if (y == 0) { l.put(u, m, x, 0); l.put(u, m, x, 1); l.put(u, m, x - 1, 0); l.put(u, m, x - 1, 1); }
    else if (x == 0) { l.put(u, m, 0, y); l.put(u, m, 1, y); l.put(u, m, 0, y - 1); }
    else { l.put(u, m, x, y); l.put(u, m, x, y - 1); l.put(u, m, x - 1, y); }
    return;
  }
  if (rect) {
    l.put(u, m, x, y - 1);
    l.put(u, m, x - 1, y);
    if (twice_w && x == xe) l.put(u, m, x - 1, y);
    l.put(u, m, x, y);
    l.put(u, m, x + 1, y);
    l.put(u, m, x, y + 1);
    return;
  }
  const int r = y % 4;
  const int up = (r == 1 || r == 2) ? 0 : -1, down = (r == 0 || r == 1) ? -1 : 0;
  l.put(u, m, x + up, y - 1);
  l.put(u, m, x + up + 1, y - 1);
  l.put(u, m, x - 1, y);
  l.put(u, m, x, y);
  l.put(u, m, x + 1, y);
  l.put(u, m, x + down, y + 1);
  l.put(u, m, x + down + 1, y + 1);
}

// the k-th smallest of l.v[0..n), by counting: any exact order statistic equals the reference's sorted table entry
__device__ __forceinline__ float umat_kth(const UmatList &l, int k) {
  float out = l.v[0];
#pragma unroll
  for (int a = 0; a < 7; a++) {
    if (a >= l.n) break;
    int less = 0, equal = 0;
#pragma unroll
    for (int b = 0; b < 7; b++) {
      if (b >= l.n) break;
      less += l.v[b] < l.v[a] ? 1 : 0;
      equal += l.v[b] == l.v[a] ? 1 : 0;
    }
    if (less <= k && k < less + equal) out = l.v[a];
  }
  return out;
}

// =====================================================================================
// K-umat-units: one thread per unit position (even x, even y); reads odd positions only, so it runs in place
// =====================================================================================
__global__ __launch_bounds__(256) void k_umat_units(UmatDims m, float *__restrict__ u) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(m.mx) * m.my) return;
  const int x = 2 * static_cast<int>(t % m.mx), y = 2 * static_cast<int>(t / m.mx);
  UmatList l;
  umat_unit_list(u, m, x, y, l);
  float r;
  if (l.n & 1) r = umat_kth(l, l.n / 2);
  else r = static_cast<float>((static_cast<double>(umat_kth(l, l.n / 2 - 1)) + static_cast<double>(umat_kth(l, l.n / 2))) / 2.0);
  u[static_cast<int64_t>(y) * m.ux + x] = r;
}

// =====================================================================================
// K-umat-minmax: bit patterns of the smallest and the largest entry (entries are >= +0, so their bit patterns order as
// unsigned integers); mm[0] preset to FLT_MAX's bits, mm[1] to 0.  A NaN entry wins no comparison in the reference.
// blockDim.x == 256; a grid-stride loop, so a few workgroups do.
// =====================================================================================
__global__ __launch_bounds__(256) void k_umat_minmax(const float *__restrict__ u, int64_t count, uint32_t *__restrict__ mm) {
  uint32_t lo = FLT_MAX_BITS, hi = 0;
  for (int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; t < count;
       t += static_cast<int64_t>(gridDim.x) * blockDim.x) {
    const float v = u[t];
    if (v != v) continue;
    const uint32_t b = __float_as_uint(v);
    lo = b < lo ? b : lo;
    hi = b > hi ? b : hi;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t ol = __shfl_xor(lo, off, WAVE), oh = __shfl_xor(hi, off, WAVE);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  __shared__ uint32_t part[2][4];                     // one pair of atomics per workgroup: they all hit the same two words
  if ((threadIdx.x & 63) == 0) {
    part[0][threadIdx.x >> 6] = lo;
    part[1][threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < 4; w++) {
      lo = part[0][w] < lo ? part[0][w] : lo;
      hi = part[1][w] > hi ? part[1][w] : hi;
    }
    atomicMin(mm, lo);
    atomicMax(mm + 1, hi);
  }
}

// K-umat-scale: u = 1.0 - (u - min) / bw in double, stored as float (map.c:493-497)
__global__ __launch_bounds__(256) void k_umat_scale(float *__restrict__ u, int64_t count, double lo, double bw) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= count) return;
  u[t] = static_cast<float>(1.0 - (static_cast<double>(u[t]) - lo) / bw);
}

// K-umat-average / K-umat-median: one thread per entry, out of place
__global__ __launch_bounds__(256) void k_umat_average(UmatDims m, const float *__restrict__ u, float *__restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(m.ux) * m.uy) return;
  UmatList l;
  umat_filter_list(u, m, static_cast<int>(t % m.ux), static_cast<int>(t / m.ux), false, l);
  float sum = l.v[0];
#pragma unroll
  for (int a = 1; a < 7; a++)
    if (a < l.n) sum = sum + l.v[a];
  out[t] = static_cast<float>(static_cast<double>(sum) / static_cast<double>(l.n));
}
__global__ __launch_bounds__(256) void k_umat_median(UmatDims m, const float *__restrict__ u, float *__restrict__ out) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= static_cast<int64_t>(m.ux) * m.uy) return;
  UmatList l;
  umat_filter_list(u, m, static_cast<int>(t % m.ux), static_cast<int>(t / m.ux), true, l);
  out[t] = umat_kth(l, l.n / 2);
}

#endif  // SOMHIP_UMAT_DEFINE

}  // namespace somhip
