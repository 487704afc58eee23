// somhip.hip -- C ABI (include/somhip.h) of the MI355X SOM/LVQ engine: host control
// of the gfx950 kernels in kernels.hpp.  No CPU fallback: every entry point runs on
// the GPU or fails with a message.
#include "../../include/somhip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.hpp"
#include "schedule.hpp"

using namespace somhip;

// ---------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}
#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail("%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)
#define CHK(expr)          \
  do {                     \
    int rc_ = (expr);      \
    if (rc_) return rc_;   \
  } while (0)

// No C++ exception may cross the C ABI (the header promises "nothing here aborts"): every extern "C" body is a
// function-try-block that ends in one of these.  The HIP runtime itself throws on some misuse (a destroyed
// stream handle gave std::bad_variant_access out of hipStreamSynchronize).
static int abi_caught(const char *who) {
  try { throw; }
  catch (const std::exception &ex) { return fail("%s: C++ exception: %s", who, ex.what()); }
  catch (...) { return fail("%s: unknown C++ exception", who); }
}
#define ABI_CATCH(name) catch (...) { return abi_caught(#name); }
#define ABI_CATCH_VOID(name) catch (...) { (void)abi_caught(#name); }

extern "C" const char *somhip_last_error(void) { return g_err.c_str(); }
extern "C" int somhip_version(void) { return SOMHIP_VERSION; }

// ---------------------------------------------------------------------------------
// kernel ids for the timing table
// ---------------------------------------------------------------------------------
// the list: X(id, the name somhip_kernel_name reports); a new kernel id goes at its end
#define SOMHIP_KERNEL_IDS(X) \
  X(SCAN_EXACT, "k_scan_exact") X(SOM_UPDATE_RUN, "k_som_update_run") X(SOM_ONLINE_STEP, "k_som_online_step") \
  X(LVQ_ONLINE_STEP, "k_lvq_online_step") X(PACK_SAMPLES, "k_pack_samples") X(MERGE_TOPK, "k_merge_topk") \
  X(SCAN_MASKED, "k_scan_masked") X(LAYOUT, "k_layout") X(DECODE, "k_decode_winners") \
  X(DIST_MFMA, "k_dist_mfma") X(RERANK, "k_rerank") X(NORMS, "k_norms_tau") \
  X(MEMBERS, "k_som_members") X(RERANK_SELECT, "k_rerank_select") X(RERANK_PAIRS, "k_rerank_pairs") \
  X(DIST_MFMA_BF16, "k_dist_mfma_bf16") X(LVQ_BATCH_APPLY, "k_lvq_batch_apply") X(SOM_UPDATE_BUBBLE_S, "k_som_update_bubble_s") \
  X(LVQ_COMPONENTS, "k_lvq_components") X(SOM_UPDATE_GEMM, "k_som_update_gemm") X(DIST_L2, "k_dist_l2") \
  X(L2_SELECT, "k_l2_select") X(SAMMON_DIST, "k_sammon_dist") X(SAMMON_SWEEP, "k_sammon_sweep") \
  X(SAMMON_CENTRE, "k_sammon_centre") X(SAMMON_ERROR, "k_sammon_error") X(CLASS_NEAREST, "k_class_nearest") \
  X(UMAT_DIST, "k_umat_dist") X(UMAT_UNITS, "k_umat_units") X(UMAT_MINMAX, "k_umat_minmax") \
  X(UMAT_SCALE, "k_umat_scale") X(UMAT_AVERAGE, "k_umat_average") X(UMAT_MEDIAN, "k_umat_median")
enum KernelId {
#define X(id, name) KID_##id,
  SOMHIP_KERNEL_IDS(X)
#undef X
  KID_COUNT
};
static const char *kKernelNames[KID_COUNT] = {
#define X(id, name) name,
  SOMHIP_KERNEL_IDS(X)
#undef X
};
// The table above is what somhip_kernel_count / somhip_kernel_name publish, and it is closed: callers index it and select
// from it by bit.  Kernels added since are timed by LaunchTimer all the same, under ids that follow the table; an entry
// point of their own reports them (somhip_mapset_timing, somhip_knn_timing, somhip_knn_vote_timing, somhip_map_quality_timing,
// somhip_batchmap_timing, somhip_conn_timing, somhip_distortion_timing, somhip_glvq_timing, somhip_ng_timing,
// somhip_grlvq_timing, somhip_gmlvq_timing, somhip_rslvq_timing, somhip_ng_dense_timing).  somhip_timing_select's mask has one bit per id up to
// 63; the ids from 64 on are outside it and are timed whenever timing is on.
enum TimedOnlyId { KID_MAPSET_TRAIN = KID_COUNT, KID_MAPSET_WINNERS, KID_KNN_DIST, KID_KNN_SELECT, KID_KNN_VOTE, KID_QUALITY_PAIRS,
                   KID_QUALITY_UNITS, KID_BATCHMAP_GROUP, KID_BATCHMAP_SUMS, KID_BATCHMAP_COMBINE, KID_CONN_KEYS, KID_CONN_SORT,
                   KID_CONN_RUNS, KID_CONN_MERGE, KID_DISTORTION_GROUP, KID_DISTORTION_SUMS, KID_DISTORTION_EVALUATE, KID_GLVQ_SEARCH,
                   KID_GLVQ_TERMS, KID_GLVQ_SUMS, KID_GLVQ_UPDATE, KID_NG_GROUP, KID_NG_SUMS, KID_NG_UPDATE,
                   KID_GRLVQ_SEARCH, KID_GRLVQ_SUMS, KID_GRLVQ_RELEVANCE, KID_GRLVQ_UPDATE,
                   KID_GMLVQ_PROJECT, KID_GMLVQ_GRAD, KID_GMLVQ_UPDATE,
                   KID_RSLVQ_DIST, KID_RSLVQ_POSTERIOR, KID_RSLVQ_SUMS, KID_RSLVQ_UPDATE,
                   KID_NG_DENSE_DIST, KID_NG_DENSE_WEIGHTS, KID_NG_DENSE_SUMS, KID_TIMED };
static_assert(KID_RSLVQ_DIST == 64, "the ids somhip_timing_select's mask can name end with K12's");
extern "C" int somhip_kernel_count(void) { return KID_COUNT; }
extern "C" const char *somhip_kernel_name(int i) { return (i >= 0 && i < KID_COUNT) ? kKernelNames[i] : ""; }

constexpr int64_t ONLINE_CHUNK = 1024;   // iterations per captured graph

struct OnlineGraphKey {
  const void *tiles; int64_t n; int d; int patch_w; int64_t row_offset; int xdim; int topol;
  const void *rows; const void *mask; const void *slot; const void *sc; const void *rowidx; bool G, M;
  bool operator==(const OnlineGraphKey &o) const {
    return tiles == o.tiles && n == o.n && d == o.d && patch_w == o.patch_w && row_offset == o.row_offset &&
           xdim == o.xdim && topol == o.topol && rows == o.rows && mask == o.mask && slot == o.slot && sc == o.sc &&
           rowidx == o.rowidx && G == o.G && M == o.M;
  }
};

// Device scratch of an engine (scratch / engine_scratch): one buffer per slot, grown on demand and kept.  The owners of a slot
// never hold it at the same time; the stages named below hold their slots together.
enum ScratchSlot {
  SLOT_STAGE = 0,          // staging of codebook upload / download; the SOM update's group order (k_order_groups);
                           // the class-ordered row tiles of somhip_class_nearest_later (which also holds SLOT_SAMPLES for the
                           // mask tiles, SLOT_CALL_A / _B for order and segment ends, SLOT_PARTIAL / SLOT_PAIRS for its results)
  SLOT_SAMPLES,            // the packed sample tiles of a scan: direct scan, or the pre-filter from prepare to level 2
  SLOT_PARTIAL,            // partial top-K lists (top-K scans and re-rank), the LVQ online loop's, the online SOM's rows
  SLOT_CALL_A,             // a host call's own array around the scans it runs: keys, LVQ candidates, column sums;
                           // somhip_umatrix: the matrix (SLOT_CALL_B its out-of-place copy, SLOT_PARTIAL min and max);
                           // somhip_planes: the grey levels (SLOT_PARTIAL the slabs' keys, SLOT_CALL_B lo and hi)
  SLOT_CALL_B,             // ... and its second one: step scalars, LvqStep, column counts, products
  SLOT_TAU,                // pre-filter: per-sample window, from prepare to the re-rank
  SLOT_WMIN,               // pre-filter: per (group, sample) minimum, from level 1 / one level to the re-rank
  SLOT_WMASK,              // pre-filter: per (group, sample) candidate mask, from level 2 / one level to the re-rank
  SLOT_MEMBER_XY,          // SOM update: the winners' lattice positions
  SLOT_MEMBER_COUNT,       // SOM update: members per row group
  SLOT_MEMBER_LIST,        // SOM update: the member lists
  SLOT_PAIRS,              // top-1 re-rank: candidate pairs in segments (bind_rerank_pairs); top-K re-rank: its pair list
  SLOT_RERANK_COUNT,       // pre-filter: re-rank counters preset in pf_prepare, from prepare to the re-rank
  SLOT_LVQ_FINAL,          // exact LVQ batches: the final keys
  SLOT_XBOUND,             // shard exchange: the deltas behind the exchanged bounds, from begin to finish
  SLOT_TOPK_SPAN,          // top-K re-rank: each sample's span of the pair list
  SLOT_LVQ_MOD,            // exact LVQ batch (lvq_batch_bufs, with the ten slots below): rows it modified
  SLOT_LVQ_RHO,            // ... sample norms, rates, the OLVQ1 rate bound
  SLOT_LVQ_ADJ,            // ... the pair relation
  SLOT_LVQ_COMP,           // ... samples per component
  SLOT_LVQ_OUT,            // ... the batch's verdict
  SLOT_LVQ_STAGE_ROWS,     // ... staged rows
  SLOT_LVQ_STAGE_ROWID,    // ... their row ids
  SLOT_LVQ_STAGE_TA,       // ... their rates
  SLOT_LVQ_CAND_LAB,       // ... the candidates' labels
  SLOT_LVQ_CAND_TA,        // ... the candidates' rates
  SLOT_L2_STATE,           // two-level pre-filter: level 1's window and minimum, level 2's counts, from prepare to the re-rank
  SLOT_L2_LIST,            // two-level pre-filter: level 2's group lists, from level 1 to the re-rank (k_rerank_select_lists)
  SLOT_LVQ_CTL,            // exact LVQ loop: its control block
  SLOT_TOPK_GROUPS,        // top-K re-rank by row group: the groups' lists and the passes (bind_topk_groups)
  SLOT_TAIL_START,         // GEMM update: where each group's list tail starts
  SLOT_SAMPLE_ROWS,        // two-level pre-filter: the sample-major copy of the tiles, from prepare to level 2
  SLOT_L2_OUT,             // two-level pre-filter, nearest row: level 2's minimum and mask of every list entry at the entry's
                           // own slot, from level 2 to the re-rank's selection (k_rerank_select_lists)
  SLOT_KNN_DIST,           // wide k-NN: the distances of a chunk of samples to every row, from the distance stage to the select
  SLOT_QUALITY,            // somhip_map_quality, somhip_map_connectivity: the run's qsum, totals and hits, around the searches of its chunks (SLOT_CALL_A the
                           // chunk's keys, SLOT_CALL_B its per-sample terms, units and distances)
  SLOT_BATCHMAP,           // the batch map (host_batchmap.inc): per unit -- the sums and counts, the gaussian table, hits and starts
  SLOT_BATCHMAP_LIST,      // ... per sample -- winners, sample numbers, their sorted copies, the sort's room (SLOT_CALL_A the
                           // chunk's keys, SLOT_CALL_B its distances)
  SLOT_GLVQ,               // batch GLVQ (host_glvq.inc): per row -- the sums of both roles, cost, counts and starts, the counters
  SLOT_GLVQ_LIST,          // ... per sample -- the two keys, xi, f, winners, sample numbers, lists, the remainder, the sort's room
                           // (SLOT_SAMPLES the class-wise scan's sample tiles; the list route's top-8 search holds its own slots)
  SLOT_NGAS,               // batch neural gas (host_ngas.inc): per unit -- [S | W], the weight table, the counts, a segment's counts and starts
  SLOT_NGAS_LIST,          // ... per (sample, rank) pair of a segment -- units, packed values, their sorted copies, the sort's room
                           // (SLOT_CALL_A the chunk's keys, SLOT_CALL_B its rank-0 distances)
  SLOT_GRLVQ,              // batch GRLVQ (host_grlvq.inc) beside SLOT_GLVQ and SLOT_GLVQ_LIST: the relevance sums of both roles per
                           // row and component, the relevance gradient, the relevance vector as a padded float4 tile
  SLOT_GMLVQ,              // batch GMLVQ (host_gmlvq.inc) beside SLOT_GLVQ and SLOT_GLVQ_LIST: the projected storage tiles and sample
                           // tiles, K9's g and P per row, the gradient of Omega, Omega and its transpose
  SLOT_GMLVQ_PART,         // ... the gradient's partial sums per block of samples; the public projection's row-major output
  SLOT_RSLVQ,              // batch RSLVQ (host_rslvq.inc): [G | c] per row, and per sample cost, P(y | x) and the correct flag
  SLOT_RSLVQ_Q,            // ... the posterior coefficients of a chunk of samples (SLOT_KNN_DIST the chunk's distances, SLOT_SAMPLES
                           // its sample tiles)
  SLOT_NGAS_DENSE,         // dense batch neural gas (host_ngas_dense.inc) beside SLOT_NGAS's [S | W]: the epoch's weight table, one
                           // double per row, and the run's rank-0 distances (SLOT_RSLVQ_Q the chunk's weights Q, SLOT_KNN_DIST its
                           // distances, SLOT_SAMPLES its sample tiles; the ranks stage: SLOT_CALL_A ranks, SLOT_CALL_B distances by unit)
  SLOT_COUNT
};

// the kernels whose dynamic LDS limit an engine raises before their first launch (raise_lds_limit): bits of lds_raised
enum LdsKernel { LDS_LVQ_APPLY, LDS_LVQ_APPLY_MASKED, LDS_LVQ_COMPONENTS, LDS_DIST_L2, LDS_L1_RING, LDS_PREP_ROWMAJOR,
                 LDS_MAPSET_TRAIN /* + 2 GAUSS + MASKED: four bits */, LDS_MAPSET_WINNERS = LDS_MAPSET_TRAIN + 4 /* + MASKED: two bits */ };
constexpr int PIN_RING = 4;       // pinned staging buffers of pin_acquire, a power of two
constexpr int LVQ_EV_RING = 8;    // batches of the exact LVQ loop in flight (lvq_train_batched)

enum XcState { XC_NONE, XC_BEGUN, XC_REFINED };   // a shard-exchanged search: the last of its calls that ran

struct somhip_engine {
  int device = 0;
  hipStream_t stream = nullptr;
  bool timing = false;
  uint64_t timing_mask = ~0ull;              // which kernel ids get events when timing is on
  int scan_mode = SOMHIP_SCAN_MFMA_BF16;
  int update_mode = SOMHIP_UPDATE_EXACT;
  unsigned long long *d_stats = nullptr;     // [STAT_WORDS] the statistics block (device; kernels/common.hpp StatWord)
  uint64_t samples_searched = 0;
  // somhip_shard_winner_begin / _refine / _finish: which search is under way on this engine, and how far it got
  int xc_phase = 0;                          // XC_NONE, XC_BEGUN, XC_REFINED
  const void *xc_cb = nullptr, *xc_ds = nullptr;
  int64_t xc_first = 0, xc_count = 0;
  uint64_t lvq_batches = 0, lvq_samples = 0;   // exact batched LVQ: rescans and samples
  uint64_t lvq_stop_list = 0, lvq_stop_cache = 0, lvq_cycles[4] = {0, 0, 0, 0};   // batches ended by an exhausted candidate list / a full cache
  int64_t lvq_batch_hint = 256;                   // batch size the exact LVQ engine starts its next call with
  uint64_t lvq_components = 0, lvq_largest = 0;   // independent components walked, and the sum of the largest one's size per batch
  // ring of pinned host staging buffers for per-batch scalars (H2D without a host sync)
  void *pin_buf[PIN_RING] = {nullptr};
  size_t pin_bytes[PIN_RING] = {0};
  hipEvent_t pin_ev[PIN_RING] = {nullptr};
  int pin_next = 0;
  hipGraphExec_t online_graph_exec = nullptr;   // one chunk of k_som_online_step launches
  OnlineGraphKey online_graph_key{};
  struct Pending { int kid; hipEvent_t a, b; };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  int64_t launches[KID_TIMED] = {0};
  double total_ms[KID_TIMED] = {0};
  // reusable device scratch
  void *scratch[SLOT_COUNT] = {nullptr};
  size_t scratch_bytes[SLOT_COUNT] = {0};
  // the mirrors created on this engine: destroying the engine first releases their device memory and orphans
  // them (their own destroy then only frees the host struct; any other call on them fails with a message)
  std::vector<somhip_codebook *> codebooks;
  std::vector<somhip_dataset *> datasets;
  std::vector<somhip_mapset *> mapsets;
  std::vector<somhip_conn *> conns;
  std::vector<somhip_distortion *> distortions;
  unsigned lds_raised = 0;                     // bit LdsKernel: that kernel's dynamic LDS limit is raised on this device
  int n_cus = 0;                               // compute units of the device (grid of the persistent kernels)
  LvqCtl *lvq_hctl = nullptr;                  // pinned: read-backs of the LVQ batch loop's control block, one per batch in flight
  hipEvent_t lvq_ev[LVQ_EV_RING] = {nullptr};
  unsigned long long *lazy_hflag = nullptr;    // pinned: read-back of STAT_LAZY_SHORT, one per lazy run of som_train_batched
};

static int check_engine(const somhip_engine *e, const char *who) { return e ? 0 : fail("%s: null engine", who); }

static int engine_scratch(somhip_engine *e, ScratchSlot slot, size_t bytes, void **out) {
  if (e->scratch_bytes[slot] < bytes) {
    if (e->scratch[slot]) HIPCHK(hipFree(e->scratch[slot]));
    e->scratch[slot] = nullptr;
    e->scratch_bytes[slot] = 0;
    size_t want = std::max(bytes, (size_t)4096);
    HIPCHK(hipMalloc(&e->scratch[slot], want));
    e->scratch_bytes[slot] = want;
  }
  *out = e->scratch[slot];
  return 0;
}
template <class T>   // ... as room for `count` elements of T
static int scratch(somhip_engine *e, ScratchSlot slot, size_t count, T **out) {
  return engine_scratch(e, slot, sizeof(T) * count, reinterpret_cast<void **>(out));
}
// once per engine (= per device, not per process) and before the kernel's first launch: more dynamic LDS than the default limit
static int raise_lds_limit(somhip_engine *e, LdsKernel which, const void *kernel, size_t bytes) {
  if ((e->lds_raised >> which) & 1u) return 0;
  HIPCHK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  e->lds_raised |= 1u << which;
  return 0;
}

template <class T> struct identity { using type = T; };   // T in a context no template argument is deduced from

// Copies of `count` elements of T on the engine's stream: the byte count follows from the pointers' type.  Asynchronous
// unless the name says otherwise; to_host_sync also waits for the stream (everything queued before the copy included).
template <class T>
static int copy_async(somhip_engine *e, T *dst, const T *src, size_t count, hipMemcpyKind kind) {
  HIPCHK(hipMemcpyAsync(dst, src, sizeof(T) * count, kind, e->stream));
  return 0;
}
template <class T> static int to_host(somhip_engine *e, T *dst, const typename identity<T>::type *src, size_t count) {
  return copy_async(e, dst, src, count, hipMemcpyDeviceToHost);
}
template <class T> static int to_device(somhip_engine *e, T *dst, const typename identity<T>::type *src, size_t count) {
  return copy_async(e, dst, src, count, hipMemcpyHostToDevice);
}
template <class T> static int on_device(somhip_engine *e, T *dst, const typename identity<T>::type *src, size_t count) {
  return copy_async(e, dst, src, count, hipMemcpyDeviceToDevice);
}
template <class T> static int to_host_sync(somhip_engine *e, T *dst, const typename identity<T>::type *src, size_t count) {
  CHK(to_host(e, dst, src, count));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

// next pinned staging buffer of the ring (waits only if its previous copy is still in flight)
static int pin_acquire(somhip_engine *e, size_t bytes, void **host, int *slot) {
  int i = e->pin_next;
  e->pin_next = (i + 1) & (PIN_RING - 1);
  if (!e->pin_ev[i]) HIPCHK(hipEventCreateWithFlags(&e->pin_ev[i], hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(e->pin_ev[i]));
  if (e->pin_bytes[i] < bytes) {
    if (e->pin_buf[i]) HIPCHK(hipHostFree(e->pin_buf[i]));
    e->pin_buf[i] = nullptr; e->pin_bytes[i] = 0;
    size_t want = std::max(bytes, (size_t)65536);
    HIPCHK(hipHostMalloc(&e->pin_buf[i], want, hipHostMallocDefault));
    e->pin_bytes[i] = want;
  }
  *host = e->pin_buf[i];
  *slot = i;
  return 0;
}
template <class T>   // (`count` elements of T: what the caller wrote into the buffer)
static int pin_upload(somhip_engine *e, int slot, T *dev, size_t count) {
  CHK(to_device(e, dev, static_cast<const T *>(e->pin_buf[slot]), count));
  HIPCHK(hipEventRecord(e->pin_ev[slot], e->stream));
  return 0;
}

static int timing_flush(somhip_engine *e) {
  if (e->pending.empty()) return 0;
  HIPCHK(hipStreamSynchronize(e->stream));
  for (auto &p : e->pending) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
    e->launches[p.kid]++;
    e->total_ms[p.kid] += ms;
    e->pool.push_back(p.a);
    e->pool.push_back(p.b);
  }
  e->pending.clear();
  return 0;
}
// What every somhip_*_timing entry point answers with: the launches and the HIP-event milliseconds of `count` kernel ids
// since somhip_timing_reset, in the order the entry point's header gives
static int stage_timing(somhip_engine *e, const char *who, const int *kid, int count, int64_t *launches, double *total_ms) {
  CHK(check_engine(e, who));
  if (!launches || !total_ms) return fail("%s: null output", who);
  CHK(timing_flush(e));
  for (int i = 0; i < count; i++) { launches[i] = e->launches[kid[i]]; total_ms[i] = e->total_ms[kid[i]]; }
  return 0;
}

struct LaunchTimer {   // HIP events on the engine's own stream around one launch (kid < 0: not timed)
  somhip_engine *e;
  int kid;
  hipEvent_t a = nullptr, b = nullptr;
  bool on = false;
  LaunchTimer(somhip_engine *e_, int kid_) : e(e_), kid(kid_) {
    if (kid_ < 0 || !e->timing || (kid_ < 64 && !((e->timing_mask >> kid_) & 1ull))) return;
    auto get = [&](hipEvent_t *ev) {
      if (!e->pool.empty()) { *ev = e->pool.back(); e->pool.pop_back(); return true; }
      return hipEventCreate(ev) == hipSuccess;
    };
    if (get(&a) && get(&b)) { on = true; (void)hipEventRecord(a, e->stream); }
  }
  ~LaunchTimer() {
    if (!on) return;
    (void)hipEventRecord(b, e->stream);
    e->pending.push_back({kid, a, b});
    if (e->pending.size() >= 2048) (void)timing_flush(e);
  }
};

// Every kernel launch of the engine: on its stream, checked at once, a failure reported under the kernel's name.  The
// arguments convert to the kernel's own parameter types (the pack is not deduced from them), so a call site casts nothing
// and writes nullptr plainly; a kernel's default arguments do not reach through the pointer and are spelled out.
template <class... P>
static int launch(somhip_engine *e, const char *name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes,
                  typename identity<P>::type... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, e->stream, args...);
  const hipError_t err = hipGetLastError();
  return err == hipSuccess ? 0 : fail("%s: launch failed: %s", name, hipGetErrorString(err));
}
template <class... P>   // ... as the one launch of a LaunchTimer scope
static int launch_timed(somhip_engine *e, int kid, const char *name, void (*kernel)(P...), dim3 grid, dim3 block,
                        size_t lds_bytes, typename identity<P>::type... args) {
  LaunchTimer t(e, kid);
  return launch(e, name, kernel, grid, block, lds_bytes, args...);
}
#define LAUNCH(e, kernel, ...) launch(e, #kernel, kernel, __VA_ARGS__)
#define LAUNCH_TIMED(e, kid, kernel, ...) launch_timed(e, kid, #kernel, kernel, __VA_ARGS__)

// ---------------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------------
static void codebook_release(somhip_codebook *cb);   // device memory of a mirror (defined with the mirrors below)
static void dataset_release(somhip_dataset *ds);
static void mapset_release(somhip_mapset *ms);
static void conn_release(somhip_conn *c);
static void distortion_release(somhip_distortion *st);

extern "C" int somhip_engine_create(int device, somhip_engine **out) try {
  if (!out) return fail("somhip_engine_create: null out");
  int ndev = 0;
  hipError_t er = hipGetDeviceCount(&ndev);
  if (er != hipSuccess || ndev <= 0)
    return fail("somhip_engine_create: no HIP device available (%s) -- this engine has no CPU path",
                er == hipSuccess ? "device count 0" : hipGetErrorString(er));
  if (device < 0 || device >= ndev) return fail("somhip_engine_create: device %d out of range (%d)", device, ndev);
  HIPCHK(hipSetDevice(device));
  somhip_engine *e = new somhip_engine();
  e->device = device;
  auto init = [&]() -> int {
    HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
    HIPCHK(hipMalloc((void **)&e->d_stats, STAT_WORDS * sizeof(unsigned long long)));
    HIPCHK(hipMemset(e->d_stats, 0, STAT_WORDS * sizeof(unsigned long long)));
    if (const char *um = getenv("SOMHIP_UPDATE_MODE")) e->update_mode = strcmp(um, "gemm") == 0 ? SOMHIP_UPDATE_GEMM : SOMHIP_UPDATE_EXACT;
    return 0;
  };
  if (int rc = init()) { somhip_engine_destroy(e); return rc; }
  *out = e;
  return 0;
} ABI_CATCH(somhip_engine_create)
extern "C" void somhip_engine_destroy(somhip_engine *e) try {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  // mirrors that outlive their engine become orphans: their device memory goes now, their handles stay valid
  // for somhip_codebook_destroy / somhip_dataset_destroy (any order of the destroy calls is fine)
  for (auto *cb : e->codebooks) codebook_release(cb);     // (these also clear the mirror's engine pointer)
  for (auto *ds : e->datasets) dataset_release(ds);
  for (auto *ms : e->mapsets) mapset_release(ms);
  for (auto *c : e->conns) conn_release(c);
  for (auto *st : e->distortions) distortion_release(st);
  for (auto &p : e->pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
  for (auto ev : e->pool) (void)hipEventDestroy(ev);
  for (int i = 0; i < SLOT_COUNT; i++) if (e->scratch[i]) (void)hipFree(e->scratch[i]);
  if (e->d_stats) (void)hipFree(e->d_stats);
  if (e->online_graph_exec) (void)hipGraphExecDestroy(e->online_graph_exec);
  for (int i = 0; i < PIN_RING; i++) {
    if (e->pin_buf[i]) (void)hipHostFree(e->pin_buf[i]);
    if (e->pin_ev[i]) (void)hipEventDestroy(e->pin_ev[i]);
  }
  if (e->lvq_hctl) (void)hipHostFree(e->lvq_hctl);
  if (e->lazy_hflag) (void)hipHostFree(e->lazy_hflag);
  for (int i = 0; i < LVQ_EV_RING; i++) if (e->lvq_ev[i]) (void)hipEventDestroy(e->lvq_ev[i]);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
} ABI_CATCH_VOID(somhip_engine_destroy)
extern "C" int somhip_device_count(int *count) try {
  if (!count) return fail("somhip_device_count: null argument");
  int n = 0;
  const hipError_t er = hipGetDeviceCount(&n);
  if (er != hipSuccess) { *count = 0; return fail("somhip_device_count: %s", hipGetErrorString(er)); }
  *count = n;
  return 0;
} ABI_CATCH(somhip_device_count)
extern "C" void *somhip_engine_stream(somhip_engine *e) { return e ? (void *)e->stream : nullptr; }
extern "C" int somhip_engine_sync(somhip_engine *e) try {
  CHK(check_engine(e, "somhip_engine_sync"));
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_engine_sync)
extern "C" int somhip_engine_set_scan_mode(somhip_engine *e, int mode) try {
  CHK(check_engine(e, "somhip_engine_set_scan_mode"));
  if (mode != SOMHIP_SCAN_DIRECT && mode != SOMHIP_SCAN_MFMA && mode != SOMHIP_SCAN_MFMA_BF16) return fail("somhip_engine_set_scan_mode: bad mode %d", mode);
  e->scan_mode = mode;
  return 0;
} ABI_CATCH(somhip_engine_set_scan_mode)
extern "C" int somhip_engine_set_update_mode(somhip_engine *e, int mode) try {
  CHK(check_engine(e, "somhip_engine_set_update_mode"));
  if (mode != SOMHIP_UPDATE_EXACT && mode != SOMHIP_UPDATE_GEMM) return fail("somhip_engine_set_update_mode: bad mode %d", mode);
  e->update_mode = mode;
  return 0;
} ABI_CATCH(somhip_engine_set_update_mode)
extern "C" int somhip_scan_stats(somhip_engine *e, uint64_t out[8]) try {
  CHK(check_engine(e, "somhip_scan_stats"));
  unsigned long long h[STAT_WORDS];
  CHK(to_host_sync(e, h, e->d_stats, STAT_WORDS));
  uint64_t rows = 0, pairs = 0, walked = 0;
  for (int k = 0; k < STAT_UPDATE_PAIRS; k++) { rows += h[STAT_UPDATE + 2 * k]; pairs += h[STAT_UPDATE + 2 * k + 1]; }
  for (int k = 0; k < STAT_GEMM_WALKS; k++) walked += h[STAT_GEMM_WALK + k];
  out[0] = h[STAT_RERANK_GROUPS]; out[1] = h[STAT_RERANK_ROWS]; out[2] = h[STAT_RERANK_MAX_GROUPS]; out[3] = e->samples_searched;
  out[4] = rows; out[5] = pairs; out[6] = walked; out[7] = h[STAT_L2_PAIRS];
  return 0;
} ABI_CATCH(somhip_scan_stats)
extern "C" int somhip_lvq_stats(somhip_engine *e, uint64_t out[12]) try {
  if (!e || !out) return fail("somhip_lvq_stats: null argument");
  out[0] = e->lvq_batches; out[1] = e->lvq_samples; out[2] = e->lvq_stop_list; out[3] = e->lvq_stop_cache;
  for (int k = 0; k < 4; k++) out[4 + k] = e->lvq_cycles[k];
  unsigned long long pairs = 0;                            // counted on the device (the top-k search does not wait for the host)
  uint32_t topk_counter[2] = {0, 0};                       // the last pre-filtered top-k search's pair list: [0] fill, [1] overflow
  HIPCHK(hipSetDevice(e->device));
  CHK(to_host(e, &pairs, e->d_stats + STAT_TOPK_PAIRS, 1));
  CHK(to_host_sync(e, topk_counter, reinterpret_cast<const uint32_t *>(e->d_stats + STAT_TOPK_LIST), 2));
  out[8] = e->lvq_components; out[9] = e->lvq_largest; out[10] = pairs; out[11] = topk_counter[1] != 0 ? 1 : 0;
  return 0;
} ABI_CATCH(somhip_lvq_stats)
extern "C" int somhip_timing_enable(somhip_engine *e, int on) try {
  CHK(check_engine(e, "somhip_timing_enable"));
  CHK(timing_flush(e));
  e->timing = on != 0;
  return 0;
} ABI_CATCH(somhip_timing_enable)
extern "C" int somhip_timing_select(somhip_engine *e, uint64_t kernel_mask) try {
  CHK(check_engine(e, "somhip_timing_select"));
  e->timing_mask = kernel_mask;
  return 0;
} ABI_CATCH(somhip_timing_select)
extern "C" int somhip_timing_reset(somhip_engine *e) try {
  CHK(check_engine(e, "somhip_timing_reset"));
  CHK(timing_flush(e));
  for (int i = 0; i < KID_TIMED; i++) { e->launches[i] = 0; e->total_ms[i] = 0; }
  return 0;
} ABI_CATCH(somhip_timing_reset)
extern "C" int somhip_timing_get(somhip_engine *e, int k, int64_t *launches, double *total_ms) try {
  CHK(check_engine(e, "somhip_timing_get"));
  if (k < 0 || k >= KID_COUNT) return fail("somhip_timing_get: bad kernel id %d", k);
  CHK(timing_flush(e));
  if (launches) *launches = e->launches[k];
  if (total_ms) *total_ms = e->total_ms[k];
  return 0;
} ABI_CATCH(somhip_timing_get)
extern "C" int somhip_device_alloc(somhip_engine *e, int64_t bytes, void **p) try {
  CHK(check_engine(e, "somhip_device_alloc"));
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipMalloc(p, (size_t)std::max<int64_t>(bytes, 16)));
  return 0;
} ABI_CATCH(somhip_device_alloc)
extern "C" int somhip_device_free(somhip_engine *e, void *p) try {
  CHK(check_engine(e, "somhip_device_free"));
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipFree(p));
  return 0;
} ABI_CATCH(somhip_device_free)
extern "C" int somhip_copy_to_host(somhip_engine *e, void *dst, const void *src, int64_t bytes) try {
  CHK(check_engine(e, "somhip_copy_to_host"));
  CHK(to_host_sync(e, (uint8_t *)dst, (const uint8_t *)src, (size_t)bytes));
  return 0;
} ABI_CATCH(somhip_copy_to_host)
extern "C" int somhip_copy_to_device(somhip_engine *e, void *dst, const void *src, int64_t bytes) try {
  CHK(check_engine(e, "somhip_copy_to_device"));
  CHK(to_device(e, (uint8_t *)dst, (const uint8_t *)src, (size_t)bytes));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_copy_to_device)

// ---------------------------------------------------------------------------------
// codebook / dataset mirrors
// ---------------------------------------------------------------------------------
struct somhip_codebook {
  somhip_engine *e = nullptr;
  CbView v{};
  int ydim = 0;
  int64_t n_global = 0;
  int32_t *d_labels = nullptr;     // [n] local rows
  float *d_talpha = nullptr;       // [n] OLVQ1 rates
  float *d_cn = nullptr;           // [ngroups*64] squared row norms (MFMA pre-filter)
  unsigned int *d_cnmax = nullptr; // bits of max squared norm: two words, used in turn by successive searches (pf_prepare)
  int cnmax_sel = 0;               // the word of the next search
  bool cnmax_clean = false;        // ... which is known to be zero
  uint4 *d_chi = nullptr, *d_clo = nullptr;   // bf16 hi/lo tiles [ngroups][d8][64] (bf16 pre-filter)
  bool prep_valid = false;         // d_cn / d_chi / d_clo describe the rows as they are now (set by a full k_prep_codes_bf16,
                                   // kept by the LVQ engine when it re-splits exactly the rows it corrected, cleared by every other writer: rows_written)
  float *d_rowmajor = nullptr;     // [ngroups*64][d] fp32 rows, row-major: what the exact re-rank of single rows gathers from (a row is
                                   // 4 d contiguous bytes here, 16 bytes per KiB in the tiles); written by the full k_prep_codes_bf16
  bool rowmajor_valid = false;     // ... set only together with prep_valid; cleared with it by every writer, and alone by a partial re-split (LVQ)
  double *bm_state = nullptr;      // the batch map's continued accumulation (host_batchmap.inc): [S | counts][the tail], the codebook's own
  bool bm_open = false;            // ... opened by somhip_batchmap_begin; closed by _end and by every other writer of the rows
  bool bm_moved = false;           // ... a _finish has written rows from it: no further piece until the next _begin
  bool bm_missing = false;         // ... the form of bm_state: [S | C] of somhip_batchmap_missing_begin, a count per component (one state, one form)
  double *gl_state = nullptr;      // batch GLVQ's continued accumulation (host_glvq.inc): [Sp | sp][Sm | sm][cost][np][nm][the tail], the codebook's own
  bool gl_open = false;            // ... opened by somhip_glvq_begin; closed by _end and by every other writer of the rows
  bool gl_moved = false;           // ... somhip_glvq_finish has written rows from it: no further piece until the next _begin
};
struct somhip_dataset {
  somhip_engine *e = nullptr;
  const float *d_rows = nullptr;
  bool owns_rows = false;
  int64_t n = 0;
  int d = 0;
  uint8_t *d_mask = nullptr;
  int32_t *d_labels = nullptr;       // device copy of labels, made by the first somhip_knn_vote that wants it
  uint8_t *d_all_masked = nullptr;   // device copy of all_masked, made by the first somhip_map_quality that wants it
  std::vector<uint8_t> all_masked;   // host: 1 if every component of the row is masked
  std::vector<int32_t> labels;       // host copies of the per-row scalars
  std::vector<int16_t> weight;
  std::vector<int16_t> fixed_xy;
};

// The two refusals an entry point on one mirror begins with.  args: its other pointer arguments are all there.
static int check_codebook(const somhip_codebook *cb, bool args, const char *who) {
  if (!cb || !args) return fail("%s: null argument", who);
  if (!cb->e) return fail("%s: the engine of this codebook was destroyed", who);
  return 0;
}
static int check_dataset(const somhip_dataset *ds, bool args, const char *who) {
  if (!ds || !args) return fail("%s: null argument", who);
  if (!ds->e) return fail("%s: the engine of this data set was destroyed", who);
  return 0;
}
// The codebook holds some of its rows only: a block of them (row_offset, n < n_global) or every patch_stride-th 8x8 patch
// of a map.  The interleaved kind starts at row 0 but, with patch_stride > 1, always has n < n_global as well.
static bool is_shard(const somhip_codebook *cb) { return cb->v.row_offset != 0 || cb->n_global != cb->v.n; }
// every component of this row is masked: it has no distance to anything, so no winner
static bool sample_is_empty(const somhip_dataset *ds, int64_t row) { return !ds->all_masked.empty() && ds->all_masked[(size_t)row]; }

// The rows of this codebook move, or the caller is about to move them: every open accumulation over them is over (the
// state stays allocated; _begin opens it again).  An owner that updates from its own state re-opens it behind the call.
static void close_accumulations(somhip_codebook *cb) { cb->bm_open = false; cb->gl_open = false; }
// What every writer of the rows says, in one place: the prepared copies no longer describe them, and see above
static void rows_written(somhip_codebook *cb) {
  cb->prep_valid = cb->rowmajor_valid = false;
  close_accumulations(cb);
}

static int upload_rows(somhip_codebook *cb, const float *rows) {
  somhip_engine *e = cb->e;
  rows_written(cb);
  float *stage;
  const size_t count = (size_t)cb->v.n * cb->v.d;
  CHK(scratch(e, SLOT_STAGE, count, &stage));
  CHK(to_device(e, stage, rows, count));
  CHK(LAUNCH_TIMED(e, KID_LAYOUT, k_rows_to_tiles, dim3((unsigned)cb->v.ngroups), dim3(256), 0, stage, cb->v));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
}

static int codebook_create(somhip_engine *e, const float *rows, const int32_t *labels, int64_t n_rows, int dim,
                           int topol, int neigh, int xdim, int ydim, int64_t row_offset, int64_t n_global,
                           int patch_stride, int patch_phase, somhip_codebook **out) {
  if (!e || !rows || !out) return fail("somhip_codebook_create: null argument");
  if (n_rows <= 0 || dim <= 0) return fail("somhip_codebook_create: empty codebook (%lld x %d)", (long long)n_rows, dim);
  if (n_global < row_offset + n_rows) return fail("somhip_codebook_create: shard [%lld,%lld) outside %lld rows",
                                                  (long long)row_offset, (long long)(row_offset + n_rows), (long long)n_global);
  if (n_global >= 0xFFFFFFFFll) return fail("somhip_codebook_create: more than 2^32-2 rows");
  if (topol >= SOMHIP_TOPOL_HEXA && (xdim <= 0 || ydim <= 0 || (int64_t)xdim * ydim != n_global))
    return fail("somhip_codebook_create: map %dx%d does not have %lld units", xdim, ydim, (long long)n_global);
  HIPCHK(hipSetDevice(e->device));
  somhip_codebook *cb = new somhip_codebook();
  cb->e = e;
  e->codebooks.push_back(cb);
  cb->v.n = n_rows;
  cb->v.ngroups = (n_rows + WAVE - 1) / WAVE;
  cb->v.d = dim;
  cb->v.d4 = (dim + 3) / 4;
  cb->v.row_offset = row_offset;
  cb->v.xdim = xdim > 0 ? xdim : 1;
  cb->v.topol = topol;
  cb->v.neigh = neigh;
  cb->v.patch_w = 0;
  cb->v.patch_stride = 1;
  cb->v.patch_phase = 0;
  if (patch_stride > 1) {                         // interleaved shard: patch order is part of its definition
    cb->v.patch_w = xdim / 8;
    cb->v.patch_stride = patch_stride;
    cb->v.patch_phase = patch_phase;
  } else if (topol >= SOMHIP_TOPOL_HEXA && xdim % 8 == 0 && ydim % 8 == 0 && row_offset % (8 * (int64_t)xdim) == 0 &&
      n_rows % (8 * (int64_t)xdim) == 0)
    cb->v.patch_w = xdim / 8;                     // 8x8-unit row groups (kernels.hpp CbView)
  cb->ydim = ydim;
  cb->n_global = n_global;
  size_t tile_bytes = (size_t)cb->v.ngroups * cb->v.d4 * WAVE * 4 * sizeof(float);
  auto fill = [&]() -> int {
    HIPCHK(hipMalloc((void **)&cb->v.tiles, tile_bytes));
    CHK(upload_rows(cb, rows));
    if (labels) {
      HIPCHK(hipMalloc((void **)&cb->d_labels, sizeof(int32_t) * (size_t)n_rows));
      HIPCHK(hipMemcpy(cb->d_labels, labels, sizeof(int32_t) * (size_t)n_rows, hipMemcpyHostToDevice));
    }
    return 0;
  };
  if (int rc = fill()) { somhip_codebook_destroy(cb); return rc; }
  *out = cb;
  return 0;
}

extern "C" int somhip_codebook_create(somhip_engine *e, const float *rows, const int32_t *labels,
                                      int64_t n_rows, int dim, int topol, int neigh, int xdim,
                                      int ydim, int64_t row_offset, int64_t n_global,
                                      somhip_codebook **out) try {
  return codebook_create(e, rows, labels, n_rows, dim, topol, neigh, xdim, ydim, row_offset, n_global, 1, 0, out);
} ABI_CATCH(somhip_codebook_create)

// Interleaved shards of a map: the map is cut into 8x8-unit patches, numbered row-major; shard s of S owns
// patches s, s+S, s+2S, ...  -- every shard sees every region of the map, so the neighbourhood updates of a
// batch are spread evenly over the ranks whatever the radius and wherever the winners fall (contiguous row
// blocks are not: the middle of the map is inside more neighbourhoods than its edges).
static int shard_patch_count(int xdim, int ydim, int shard_index, int shard_count, int64_t *count) {
  if (xdim <= 0 || ydim <= 0 || xdim % 8 || ydim % 8) return fail("interleaved shards need map sides that are multiples of 8 (%dx%d)", xdim, ydim);
  if (shard_count < 1 || shard_index < 0 || shard_index >= shard_count) return fail("shard %d of %d", shard_index, shard_count);
  const int64_t patches = (int64_t)(xdim / 8) * (ydim / 8);
  *count = patches > shard_index ? (patches - shard_index + shard_count - 1) / shard_count : 0;
  return 0;
}
extern "C" int somhip_shard_units(int xdim, int ydim, int shard_index, int shard_count, int64_t *units,
                                  int64_t *n_units) try {
  int64_t np = 0;
  CHK(shard_patch_count(xdim, ydim, shard_index, shard_count, &np));
  if (n_units) *n_units = np * 64;
  if (!units) return 0;
  CbView v{};
  v.xdim = xdim; v.patch_w = xdim / 8; v.patch_stride = shard_count; v.patch_phase = shard_index;
  for (int64_t r = 0; r < np * 64; r++) units[r] = shard_count == 1 ? r : (int64_t)unit_of_row(v, r);   // one shard = the whole map, unit order
  return 0;
} ABI_CATCH(somhip_shard_units)
extern "C" int somhip_codebook_create_interleaved(somhip_engine *e, const float *rows, int64_t n_rows, int dim,
                                                  int topol, int neigh, int xdim, int ydim, int shard_index,
                                                  int shard_count, somhip_codebook **out) try {
  if (topol < SOMHIP_TOPOL_HEXA) return fail("somhip_codebook_create_interleaved: maps only");
  int64_t np = 0;
  CHK(shard_patch_count(xdim, ydim, shard_index, shard_count, &np));
  if (n_rows != np * 64) return fail("somhip_codebook_create_interleaved: shard %d of %d of a %dx%d map has %lld units, not %lld",
                                     shard_index, shard_count, xdim, ydim, (long long)(np * 64), (long long)n_rows);
  return codebook_create(e, rows, nullptr, n_rows, dim, topol, neigh, xdim, ydim, 0, (int64_t)xdim * ydim,
                         shard_count > 1 ? shard_count : 1, shard_count > 1 ? shard_index : 0, out);
} ABI_CATCH(somhip_codebook_create_interleaved)
extern "C" int somhip_codebook_upload(somhip_codebook *cb, const float *rows) try {
  CHK(check_codebook(cb, rows, "somhip_codebook_upload"));
  HIPCHK(hipSetDevice(cb->e->device));
  return upload_rows(cb, rows);
} ABI_CATCH(somhip_codebook_upload)
extern "C" int somhip_codebook_download(somhip_codebook *cb, float *rows) try {
  CHK(check_codebook(cb, rows, "somhip_codebook_download"));
  somhip_engine *e = cb->e;
  HIPCHK(hipSetDevice(e->device));
  float *stage;
  const size_t count = (size_t)cb->v.n * cb->v.d;
  CHK(scratch(e, SLOT_STAGE, count, &stage));
  CHK(LAUNCH_TIMED(e, KID_LAYOUT, k_tiles_to_rows, dim3((unsigned)cb->v.ngroups), dim3(256), 0, stage, cb->v));
  CHK(to_host_sync(e, rows, stage, count));
  return 0;
} ABI_CATCH(somhip_codebook_download)
static void codebook_release(somhip_codebook *cb) {
  if (cb->v.tiles) (void)hipFree(cb->v.tiles);
  if (cb->d_labels) (void)hipFree(cb->d_labels);
  if (cb->d_talpha) (void)hipFree(cb->d_talpha);
  if (cb->d_cn) (void)hipFree(cb->d_cn);
  if (cb->d_cnmax) (void)hipFree(cb->d_cnmax);
  if (cb->d_rowmajor) (void)hipFree(cb->d_rowmajor);
  cb->d_rowmajor = nullptr;
  if (cb->d_chi) (void)hipFree(cb->d_chi);
  if (cb->d_clo) (void)hipFree(cb->d_clo);
  if (cb->bm_state) (void)hipFree(cb->bm_state);
  cb->bm_state = nullptr; cb->bm_open = false;
  if (cb->gl_state) (void)hipFree(cb->gl_state);
  cb->gl_state = nullptr; cb->gl_open = false;
  cb->v.tiles = nullptr;
  cb->d_labels = nullptr; cb->d_talpha = nullptr; cb->d_cn = nullptr; cb->d_cnmax = nullptr;
  cb->d_chi = cb->d_clo = nullptr;
  cb->e = nullptr;
}
extern "C" void somhip_codebook_destroy(somhip_codebook *cb) try {
  if (!cb) return;
  if (somhip_engine *e = cb->e) {                       // an orphan (engine destroyed first) has nothing left on the device
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    codebook_release(cb);
    e->codebooks.erase(std::remove(e->codebooks.begin(), e->codebooks.end(), cb), e->codebooks.end());
  }
  delete cb;
} ABI_CATCH_VOID(somhip_codebook_destroy)

extern "C" int somhip_dataset_create(somhip_engine *e, const float *rows, int64_t n_rows, int dim,
                                     const uint8_t *mask, const int32_t *labels,
                                     const int16_t *weight, const int16_t *fixed_xy,
                                     somhip_dataset **out) try {
  if (!e || !rows || !out) return fail("somhip_dataset_create: null argument");
  if (n_rows <= 0 || dim <= 0) return fail("somhip_dataset_create: empty data set");
  HIPCHK(hipSetDevice(e->device));
  somhip_dataset *ds = new somhip_dataset();
  ds->e = e; ds->n = n_rows; ds->d = dim; ds->owns_rows = true;
  e->datasets.push_back(ds);
  auto fill = [&]() -> int {
  size_t bytes = sizeof(float) * (size_t)n_rows * dim;
  float *dr = nullptr;
  // 16 spare bytes: wave-uniform float4 reads of the last row never leave the buffer
  HIPCHK(hipMalloc((void **)&dr, bytes + 16));
  ds->d_rows = dr;
  HIPCHK(hipMemcpy(dr, rows, bytes, hipMemcpyHostToDevice));
  if (mask) {
    bool any = false;
    ds->all_masked.assign((size_t)n_rows, 0);
    for (int64_t r = 0; r < n_rows; r++) {
      int cnt = 0;
      for (int i = 0; i < dim; i++) cnt += mask[r * dim + i] != 0;
      any |= cnt > 0;
      ds->all_masked[(size_t)r] = cnt == dim;
    }
    if (any) {
      HIPCHK(hipMalloc((void **)&ds->d_mask, (size_t)n_rows * dim));
      HIPCHK(hipMemcpy(ds->d_mask, mask, (size_t)n_rows * dim, hipMemcpyHostToDevice));
    } else {
      ds->all_masked.clear();
    }
  }
  if (labels) ds->labels.assign(labels, labels + n_rows);
  if (weight) ds->weight.assign(weight, weight + n_rows);
  if (fixed_xy) {
    // -1,-1 = no fixed point; a negative coordinate is how "none" is written, so it cannot also be a position
    for (int64_t r = 0; r < n_rows; r++)
      if ((fixed_xy[2 * r] < 0) != (fixed_xy[2 * r + 1] < 0) || fixed_xy[2 * r] < -1 || fixed_xy[2 * r + 1] < -1)
        return fail("somhip_dataset_create: fixed point (%d,%d) of row %lld: negative coordinates are not supported",
                    fixed_xy[2 * r], fixed_xy[2 * r + 1], (long long)r);
    ds->fixed_xy.assign(fixed_xy, fixed_xy + 2 * n_rows);
  }
  return 0;
  };
  if (int rc = fill()) { somhip_dataset_destroy(ds); return rc; }
  *out = ds;
  return 0;
} ABI_CATCH(somhip_dataset_create)
extern "C" int somhip_dataset_wrap_device(somhip_engine *e, const float *dev_rows, int64_t n_rows,
                                          int dim, somhip_dataset **out) try {
  if (!e || !dev_rows || !out) return fail("somhip_dataset_wrap_device: null argument");
  if (n_rows <= 0 || dim <= 0) return fail("somhip_dataset_wrap_device: empty data set");
  somhip_dataset *ds = new somhip_dataset();
  ds->e = e; ds->n = n_rows; ds->d = dim; ds->d_rows = dev_rows; ds->owns_rows = false;
  e->datasets.push_back(ds);
  *out = ds;
  return 0;
} ABI_CATCH(somhip_dataset_wrap_device)
extern "C" int somhip_dataset_generate(somhip_engine *e, uint64_t seed, int k_centres, int dim, int64_t first_row,
                                       int64_t n_rows, int32_t *centres, somhip_dataset **out) try {
  if (!e || !out) return fail("somhip_dataset_generate: null argument");
  if (k_centres <= 0 || dim <= 0 || n_rows <= 0 || first_row < 0) return fail("somhip_dataset_generate: bad shape");
  HIPCHK(hipSetDevice(e->device));
  somhip_dataset *ds = new somhip_dataset();
  ds->e = e; ds->n = n_rows; ds->d = dim; ds->owns_rows = true;
  e->datasets.push_back(ds);
  int32_t *dcen = nullptr;
  auto fill = [&]() -> int {
  float *rows = nullptr;
  HIPCHK(hipMalloc((void **)&rows, sizeof(float) * (size_t)n_rows * dim + 16));   // same 16 spare bytes as dataset_create
  ds->d_rows = rows;
  if (centres) HIPCHK(hipMalloc((void **)&dcen, sizeof(int32_t) * (size_t)n_rows));
  const int64_t total = n_rows * dim;
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
  CHK(LAUNCH_TIMED(e, KID_LAYOUT, k_gen_mixture, dim3(blocks), dim3(256), 0, seed, k_centres, dim, first_row, n_rows, rows, dcen));
  if (centres) {
    CHK(to_host_sync(e, centres, dcen, (size_t)n_rows));
    ds->labels.assign(centres, centres + n_rows);
  }
  return 0;
  };
  const int rc = fill();
  if (dcen) (void)hipFree(dcen);
  if (rc) { somhip_dataset_destroy(ds); return rc; }
  *out = ds;
  return 0;
} ABI_CATCH(somhip_dataset_generate)
extern "C" int somhip_dataset_download_rows(somhip_dataset *ds, int64_t first, int64_t count, float *rows) try {
  CHK(check_dataset(ds, rows, "somhip_dataset_download_rows"));
  if (first < 0 || count < 0 || first + count > ds->n) return fail("somhip_dataset_download_rows: rows [%lld,%lld) outside %lld",
                                                                 (long long)first, (long long)(first + count), (long long)ds->n);
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(ds->e->device));
  CHK(to_host_sync(ds->e, rows, ds->d_rows + first * ds->d, (size_t)count * ds->d));
  return 0;
} ABI_CATCH(somhip_dataset_download_rows)
static void dataset_release(somhip_dataset *ds) {
  if (ds->owns_rows && ds->d_rows) (void)hipFree((void *)ds->d_rows);
  if (ds->d_mask) (void)hipFree(ds->d_mask);
  if (ds->d_labels) (void)hipFree(ds->d_labels);
  if (ds->d_all_masked) (void)hipFree(ds->d_all_masked);
  ds->d_rows = nullptr;
  ds->d_mask = nullptr;
  ds->d_labels = nullptr;
  ds->d_all_masked = nullptr;
  ds->e = nullptr;
}
extern "C" void somhip_dataset_destroy(somhip_dataset *ds) try {
  if (!ds) return;
  if (somhip_engine *e = ds->e) {
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    dataset_release(ds);
    e->datasets.erase(std::remove(e->datasets.begin(), e->datasets.end(), ds), e->datasets.end());
  }
  delete ds;
} ABI_CATCH_VOID(somhip_dataset_destroy)

// the rest of the host side, by stage (same translation unit)
#include "host_scan.inc"
#include "host_som.inc"
#include "host_mapset.inc"
#include "host_lvq.inc"
#include "host_comm.inc"
#include "host_sammon.inc"
#include "host_class.inc"
#include "host_umat.inc"
#include "host_planes.inc"
#include "host_conn.inc"
#include "host_quality.inc"
#include "host_proto.inc"
#include "host_batchmap.inc"
#include "host_glvq.inc"
#include "host_ngas.inc"
#include "host_grlvq.inc"
#include "host_distortion.inc"
#include "host_gmlvq.inc"
#include "host_rslvq.inc"
#include "host_ngas_dense.inc"
