// kernels/map_conn.hpp -- K1c: map connectivity, the count of samples per ordered (best, second-best) unit pair, behind the
// keys of a top-2 search
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "map_quality.hpp"

namespace somhip {

// =====================================================================================
// K1c: CADJ(i, j) = the samples whose best unit is i and second-best j.  b1, b2 and "defined" are
// K1q's, from the same keys.  Integers only: every result is a count, equal wherever a run is cut.
//
//   keys     k_conn_keys, one lane per sample of a chunk: the pair as one word (b1 << ubits) | b2, ubits the bit length of
//            units - 1, CONN_NO_PAIR for a sample that is not defined; appended to the slab.
//   sort     per slab, a device radix sort of the words over bits [0, 2 ubits) (the host, rocPRIM): CONN_NO_PAIR has all of
//            them set, which no pair has (b1 != b2), so it sorts last.
//   runs     k_conn_heads flags the first word of every run of equal words; an exclusive scan of the flags (rocPRIM) numbers
//            the runs; k_conn_runs writes each run's word and start.  A run's count is the next run's start less its own.
//   merge    the table is a sorted list of (word, uint64 count) without duplicates.  k_conn_rank marks the runs whose word
//            the table does not hold; an exclusive scan counts them; k_conn_merge gives every element of either list its
//            place in the merged list: its own index, plus its rank in the other list by a binary search (for a run: among
//            the table's words; for a table entry: among the new runs, from the scan).  Every place is written once, in
//            word order, with no atomics.
// =====================================================================================
constexpr uint64_t CONN_NO_PAIR = KEY_NONE;       // the word of a sample without a defined pair
constexpr int CONN_THREADS = 256;

// the bit length of n_units - 1, at least 1: what one unit index of a pair's word takes
__host__ __device__ inline int conn_unit_bits(uint64_t n_units) {
  int bits = 1;
  while (bits < 32 && (static_cast<uint64_t>(1) << bits) < n_units) bits++;
  return bits;
}

// out[s] for sample s of the chunk (data row (first + s) % n_rows) from keys[s][stride], stride >= 2: the pair's word
// where k_quality_pairs counts the sample as topo_defined (same flags, same tests), CONN_NO_PAIR elsewhere
__global__ __launch_bounds__(CONN_THREADS) void k_conn_keys(const uint64_t *__restrict__ keys, int stride,
                                                            const uint8_t *__restrict__ all_masked, int64_t first,
                                                            int64_t n_rows, int64_t count, int64_t n_units, int ubits,
                                                            uint64_t *__restrict__ out) {
  const int64_t smp = static_cast<int64_t>(blockIdx.x) * CONN_THREADS + threadIdx.x;
  if (smp >= count) return;
  const bool searched = !(all_masked && all_masked[(first + smp) % n_rows]);
  const uint64_t k1 = keys[smp * stride], k2 = keys[smp * stride + 1];
  const uint32_t u1 = static_cast<uint32_t>(k1), u2 = static_cast<uint32_t>(k2);
  const bool has1 = searched && static_cast<uint32_t>(k1 >> 32) < FLT_MAX_BITS && u1 < n_units;
  const bool defined = has1 && static_cast<uint32_t>(k2 >> 32) < FLT_MAX_BITS && u2 < n_units;
  out[smp] = defined ? (static_cast<uint64_t>(u1) << ubits) | u2 : CONN_NO_PAIR;
}

// flag[i] = 1 where sorted[i] starts a run of equal words, i < m; flag[m] = 0, so that an exclusive scan of m + 1 flags
// ends in the number of runs.  The CONN_NO_PAIR words at the end are a run like the others.
__global__ __launch_bounds__(CONN_THREADS) void k_conn_heads(const uint64_t *__restrict__ sorted, uint32_t m,
                                                             uint32_t *__restrict__ flag) {
  const uint32_t i = blockIdx.x * CONN_THREADS + threadIdx.x;
  if (i > m) return;
  flag[i] = i < m && (i == 0 || sorted[i - 1] != sorted[i]) ? 1u : 0u;
}

enum ConnInfo { CONN_INFO_RUNS, CONN_INFO_DEFINED, CONN_INFO_WORDS };
// From the scanned flags (pos[i] = heads before i, pos[m] = all of them), m >= 1: run_key[p] and run_start[p] of every run
// p, run_start[runs] = m; info[CONN_INFO_RUNS] = the runs of pairs (those but the CONN_NO_PAIR one), info[CONN_INFO_DEFINED]
// = the words before the CONN_NO_PAIR ones.  The CONN_NO_PAIR run is the last one, so the count of every run of pairs is
// run_start[p + 1] - run_start[p].
__global__ __launch_bounds__(CONN_THREADS) void k_conn_runs(const uint64_t *__restrict__ sorted, uint32_t m,
                                                            const uint32_t *__restrict__ pos, uint64_t *__restrict__ run_key,
                                                            uint32_t *__restrict__ run_start, uint32_t *__restrict__ info) {
  const uint32_t i = blockIdx.x * CONN_THREADS + threadIdx.x;
  if (i >= m) return;
  const uint64_t k = sorted[i];
  const bool head = i == 0 || sorted[i - 1] != k;
  if (head) {
    run_key[pos[i]] = k;
    run_start[pos[i]] = i;
    if (k == CONN_NO_PAIR) info[CONN_INFO_DEFINED] = i;
  }
  if (i == m - 1) {
    const uint32_t runs = pos[m];
    run_start[runs] = m;
    info[CONN_INFO_RUNS] = k == CONN_NO_PAIR ? runs - 1 : runs;
    if (k != CONN_NO_PAIR) info[CONN_INFO_DEFINED] = m;
  }
}

// the first index of the ascending list[n] whose word is not below k (n if none is)
__device__ __forceinline__ int64_t conn_lower_bound(const uint64_t *__restrict__ list, int64_t n, uint64_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (list[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// is_new[j] = 1 where the table (table_key[n], ascending) does not hold run_key[j], j < runs; is_new[runs] = 0, so that an
// exclusive scan of runs + 1 flags ends in the number of new words
__global__ __launch_bounds__(CONN_THREADS) void k_conn_rank(const uint64_t *__restrict__ run_key, uint32_t runs,
                                                            const uint64_t *__restrict__ table_key, int64_t n,
                                                            uint32_t *__restrict__ is_new) {
  const uint32_t j = blockIdx.x * CONN_THREADS + threadIdx.x;
  if (j > runs) return;
  uint32_t f = 0;
  if (j < runs) {
    const uint64_t k = run_key[j];
    const int64_t at = conn_lower_bound(table_key, n, k);
    f = at < n && table_key[at] == k ? 0u : 1u;
  }
  is_new[j] = f;
}

// The merged table from the table (n entries) and the runs, new_pos[j] = the new runs before run j (new_pos[runs]: all of
// them).  Lane t < n moves table entry t up by the new runs below its word and adds the count of the run with its word, if
// there is one; lane n + j places run j, if it is new, behind the table entries below its word and the new runs before it.
// out_key / out_count hold n + new_pos[runs] entries afterwards and are not the table's own arrays.
__global__ __launch_bounds__(CONN_THREADS) void k_conn_merge(const uint64_t *__restrict__ table_key,
                                                             const uint64_t *__restrict__ table_count, int64_t n,
                                                             const uint64_t *__restrict__ run_key,
                                                             const uint32_t *__restrict__ run_start,
                                                             const uint32_t *__restrict__ new_pos, uint32_t runs,
                                                             uint64_t *__restrict__ out_key, uint64_t *__restrict__ out_count) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * CONN_THREADS + threadIdx.x;
  if (t < n) {
    const uint64_t k = table_key[t];
    const int64_t r = conn_lower_bound(run_key, runs, k);
    uint64_t c = table_count[t];
    if (r < runs && run_key[r] == k) c += run_start[r + 1] - run_start[r];
    const int64_t at = t + new_pos[r];
    out_key[at] = k;
    out_count[at] = c;
  } else if (t - n < runs) {
    const uint32_t j = static_cast<uint32_t>(t - n);
    if (new_pos[j + 1] == new_pos[j]) return;                 // the table holds this word: its entry took the count
    const uint64_t k = run_key[j];
    const int64_t at = conn_lower_bound(table_key, n, k) + new_pos[j];
    out_key[at] = k;
    out_count[at] = run_start[j + 1] - run_start[j];
  }
}

}  // namespace somhip
