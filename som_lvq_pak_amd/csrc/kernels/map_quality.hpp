// kernels/map_quality.hpp -- K1q: topographic error and per-unit hit counts / error sums, behind the keys of a top-2 search
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "knn_vote.hpp"

namespace somhip {

// =====================================================================================
// K1q: what a trained map's quality figures take from the two nearest units of every sample.
//
// The keys are SOMHIP_TIE_FIRST's: (distance bits, unit), ascending, so b1 is find_winner_euc's winner (lvq_pak.c:56-78:
// the lowest index among equal distances) and b2 the winner of the codebook without row b1.  An empty slot has distance
// bits >= FLT_MAX_BITS (nothing beat FLT_MAX, lvq_pak.c:56).  b1 and b2 are adjacent when lattice_sq <= 1: the units a
// bubble of radius 1 around b1 teaches (som_rout.c:489-497) -- six on a hexagonal lattice (0.25 + 0.75 = 1 exactly, the
// next value is 3), four on a rectangular one (the diagonal is 2).
//
// Two passes per chunk of samples.  The pair pass, one lane per sample, counts the totals and leaves (b1, sqrt(d1)) per
// sample.  The unit pass groups the chunk's samples by unit, data order kept inside a group, and gives every group to one
// lane, so qsum[u] is one chain of fp64 additions in data order: no float atomics, the same bits wherever the run is cut
// into chunks or calls.  (A lane per unit walking every sample of the chunk gives the same bits; it took 46 % of the call
// on a 32 x 32 map: profiles/map_quality_vs_parent.txt.)
// =====================================================================================
constexpr uint32_t QUAL_NO_UNIT = 0xFFFFFFFFu;    // the unit of a sample that counts for no unit
constexpr int QUAL_THREADS = 256;                 // the pair pass
constexpr int QUAL_CHUNK = 4096;                  // most samples of a chunk: what the unit pass sorts in LDS (64 KiB)
constexpr int QUAL_SORT_THREADS = 1024;
enum QualTotal { QUAL_SEARCHED, QUAL_TOPO_DEFINED, QUAL_TOPO_ERRORS, QUAL_TOTALS };

// Per sample s of the chunk (data row (first + s) % n_rows) from keys[s][stride], stride >= 2: unit[s] = b1, d1[s] = its
// squared distance, term[s] = sqrt((double)d1).  A sample whose all_masked flag is set (null: none is) is not searched,
// whatever its keys say: unit QUAL_NO_UNIT, d1 -1.  A searched sample without a winner has unit QUAL_NO_UNIT and d1 -1 as
// well (what somhip_find_winners reports for it).  totals[QualTotal] += the chunk's counts: one atomic per wave and word.
__global__ __launch_bounds__(QUAL_THREADS) void k_quality_pairs(const uint64_t *__restrict__ keys, int stride,
                                                                const uint8_t *__restrict__ all_masked, int64_t first,
                                                                int64_t n_rows, int64_t count, int64_t n_units, int xdim,
                                                                int topol, uint32_t *__restrict__ unit,
                                                                float *__restrict__ d1, double *__restrict__ term,
                                                                unsigned long long *__restrict__ totals) {
  const int64_t smp = static_cast<int64_t>(blockIdx.x) * QUAL_THREADS + threadIdx.x;
  const bool in_run = smp < count;
  bool searched = false, defined = false, error = false;
  if (in_run) {
    searched = !(all_masked && all_masked[(first + smp) % n_rows]);
    const uint64_t k1 = keys[smp * stride], k2 = keys[smp * stride + 1];
    const uint32_t u1 = static_cast<uint32_t>(k1), u2 = static_cast<uint32_t>(k2);
    const bool has1 = searched && static_cast<uint32_t>(k1 >> 32) < FLT_MAX_BITS && u1 < n_units;
    defined = has1 && static_cast<uint32_t>(k2 >> 32) < FLT_MAX_BITS && u2 < n_units;
    if (defined) {
      const uint32_t xd = static_cast<uint32_t>(xdim);
      error = !(lattice_sq(topol, static_cast<int>(u1 % xd), static_cast<int>(u1 / xd), static_cast<int>(u2 % xd),
                           static_cast<int>(u2 / xd)) <= 1.0f);
    }
    const float d = has1 ? __uint_as_float(static_cast<uint32_t>(k1 >> 32)) : -1.0f;
    unit[smp] = has1 ? u1 : QUAL_NO_UNIT;
    d1[smp] = d;
    term[smp] = has1 ? sqrt(static_cast<double>(d)) : 0.0;
  }
  const unsigned long long ns = __popcll(__ballot(searched)), nd = __popcll(__ballot(defined)), ne = __popcll(__ballot(error));
  if ((threadIdx.x & (WAVE - 1)) == 0) {
    if (ns) atomicAdd(totals + QUAL_SEARCHED, ns);
    if (nd) atomicAdd(totals + QUAL_TOPO_DEFINED, nd);
    if (ne) atomicAdd(totals + QUAL_TOPO_ERRORS, ne);
  }
}

// hits[u] += the chunk's samples with unit[s] == u; qsum[u] += their term[s], one addition per sample in the order of s.
// One workgroup for the chunk (count <= QUAL_CHUNK): a bitonic sort in LDS of the keys (unit, s) -- equal units end up
// side by side in the order of s, QUAL_NO_UNIT last -- then the lane at the head of every run of one unit walks the run
// from the unit's global values on.  Units differ between runs, so no two lanes touch one element.
__global__ __launch_bounds__(QUAL_SORT_THREADS) void k_quality_units(const uint32_t *__restrict__ unit,
                                                                     const double *__restrict__ term, int count,
                                                                     uint32_t *__restrict__ hits,
                                                                     double *__restrict__ qsum) {
  __shared__ uint64_t s_key[QUAL_CHUNK];
  __shared__ double s_term[QUAL_CHUNK];
  int n2 = 2;                                                 // the sorted length: a power of two >= count
  while (n2 < count) n2 <<= 1;
  for (int t = threadIdx.x; t < n2; t += QUAL_SORT_THREADS) {
    s_key[t] = t < count ? (static_cast<uint64_t>(unit[t]) << 32) | static_cast<uint32_t>(t) : KEY_NONE;
    if (t < count) s_term[t] = term[t];
  }
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n2 >> 1); t += QUAL_SORT_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t a = s_key[i], b = s_key[l];
        if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[l] = a; }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < count; i += QUAL_SORT_THREADS) {
    const uint32_t u = static_cast<uint32_t>(s_key[i] >> 32);
    if (u == QUAL_NO_UNIT || (i > 0 && static_cast<uint32_t>(s_key[i - 1] >> 32) == u)) continue;   // not the head of a run
    uint32_t h = hits[u];
    double q = qsum[u];
    for (int j = i; j < count; j++) {
      const uint64_t k = s_key[j];
      if (static_cast<uint32_t>(k >> 32) != u) break;
      h++;
      q += s_term[static_cast<uint32_t>(k)];
    }
    hits[u] = h;
    qsum[u] = q;
  }
}

}  // namespace somhip
