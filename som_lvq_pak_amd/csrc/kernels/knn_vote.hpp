// kernels/knn_vote.hpp -- K1v: the class vote of a k-NN search over the neighbours' labels, behind the keys of any route
// (part of kernels.hpp; see the notes at the top of that file)
#pragma once
#include "knn_wide.hpp"

namespace somhip {

// =====================================================================================
// K1v: what every consumer of k neighbours takes from them (knntest.c:101-108, setlabel.c:73-80, correct_by_knn
// lvq_rout.c:38-78, elimin.c:87-101): the head of the hit list after add_hit (labels.c:370-410) of the neighbours'
// labels, nearest first, and how many neighbours carry the sample's own label.
//
// The hit list stays sorted by falling count; a new label joins at the tail and a bumped entry passes only entries
// with a strictly smaller count.  So an entry reaches the head when its count first exceeds every other, and keeps it
// against later equals: the head is the label whose count FIRST reaches the final maximum M.  With
//     rank_j = #{i <= j : lab_i == lab_j}     (equality of the int32 values)
// rank_j never exceeds the final count of lab_j, so max_j rank_j = M, and the head is lab_j of the smallest j with
// rank_j = M: one minimum over the keys (~rank_j, j).
//
// One wave per sample, four samples per workgroup; lanes take neighbours lane + 64 i.  Integer work only.
// =====================================================================================
constexpr int VOTE_SAMPLES = 4;                       // samples (waves) of a workgroup
constexpr int VOTE_PER_LANE = KNN_WIDE_MAX / WAVE;    // neighbours of a lane

// out[sample] <- {label, freq, own, found} from keys[sample][stride] (ascending; the first knn count; empty slots
// sort last, so the live keys are a prefix: found of them).  inverted: the tag is ~unit (SOMHIP_TIE_KNN), else the
// unit.  cb_labels[unit - row_offset] is a row's label (n_codes of them); ds_labels (or null: own = -1) the data
// rows' own labels, sample s being data row (first + s) % n_rows.  found 0: label -1, freq 0.
__global__ __launch_bounds__(VOTE_SAMPLES * WAVE) void k_knn_vote(const uint64_t *__restrict__ keys, int stride, int knn,
                                                                  int inverted, const int32_t *__restrict__ cb_labels,
                                                                  int64_t row_offset, int64_t n_codes,
                                                                  const int32_t *__restrict__ ds_labels, int64_t first,
                                                                  int64_t n_rows, int64_t count, int4 *__restrict__ out) {
  __shared__ int32_t s_lab[VOTE_SAMPLES][KNN_WIDE_MAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t smp = static_cast<int64_t>(blockIdx.x) * VOTE_SAMPLES + wave;
  const bool in_run = smp < count;            // (a wave beyond the run keeps the barrier and votes on nothing)
  const int32_t own_lab = in_run && ds_labels ? ds_labels[(first + smp) % n_rows] : 0;
  int32_t lab[VOTE_PER_LANE];
  int found = 0, own = 0;
#pragma unroll
  for (int i = 0; i < VOTE_PER_LANE; i++) {
    const int j = lane + WAVE * i;
    bool live = false;
    lab[i] = 0;
    if (in_run && j < knn) {
      const uint64_t k = keys[smp * stride + j];
      const uint32_t tag = static_cast<uint32_t>(k);
      const int64_t row = static_cast<int64_t>(inverted ? ~tag : tag) - row_offset;
      live = static_cast<uint32_t>(k >> 32) < FLT_MAX_BITS && row >= 0 && row < n_codes;
      if (live) lab[i] = cb_labels[row];
    }
    if (live) s_lab[wave][j] = lab[i];
    found += __popcll(__ballot(live));
    own += __popcll(__ballot(live && lab[i] == own_lab));
  }
  __syncthreads();
  int rank[VOTE_PER_LANE];
#pragma unroll
  for (int i = 0; i < VOTE_PER_LANE; i++) rank[i] = 0;
  for (int t = 0; t < found; t++) {
    const int32_t l = s_lab[wave][t];         // wave-uniform address
#pragma unroll
    for (int i = 0; i < VOTE_PER_LANE; i++) rank[i] += (l == lab[i] && t <= lane + WAVE * i) ? 1 : 0;
  }
  uint64_t best = KEY_NONE;
#pragma unroll
  for (int i = 0; i < VOTE_PER_LANE; i++) {
    const int j = lane + WAVE * i;
    if (j < found) {
      const uint64_t v = (static_cast<uint64_t>(~static_cast<uint32_t>(rank[i])) << 32) | static_cast<uint32_t>(j);
      best = v < best ? v : best;
    }
  }
  best = wave_min_u64(best);
  if (lane == 0 && in_run) {
    int4 r = make_int4(-1, 0, ds_labels ? own : -1, found);
    if (found > 0) {
      r.x = s_lab[wave][static_cast<uint32_t>(best)];
      r.y = static_cast<int>(~static_cast<uint32_t>(best >> 32));
    }
    out[smp] = r;
  }
}

}  // namespace somhip
