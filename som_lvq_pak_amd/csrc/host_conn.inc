// host_conn.inc -- K1c, map connectivity: the pair table (somhip_conn) and the passes that add a run's (best, second-best)
// unit pairs to it -- the words of a chunk, and per slab the sort, the runs and the merge.  The search and the entry point
// somhip_map_connectivity are the map quality driver's (host_quality.inc).
// (included by somhip.hip: one translation unit, shared static helpers)
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

static_assert(SOMHIP_CONN_SLAB < ((int64_t)1 << 31), "a slab's positions and run counts are 32-bit words");
constexpr int64_t CONN_FIRST_CAPACITY = 1024;     // entries of a table's first buffers; doubled until a merge fits

// The table: entries [0, n) of key[cur] / count[cur], ascending by word, no word twice.  A merge writes the other pair of
// buffers and makes it the current one.  Everything below `slab` is the room of one slab, kept between calls.
struct somhip_conn {
  somhip_engine *e = nullptr;
  uint64_t *key[2] = {nullptr, nullptr}, *count[2] = {nullptr, nullptr};
  int64_t cap[2] = {0, 0};
  int cur = 0;
  int64_t n = 0;                    // entries
  uint64_t samples = 0;             // the sum of their counts
  int64_t units = 0;                // of the codebook whose pairs the table holds (n > 0)
  int ubits = 0;                    // ... and the bits of a unit in a word
  // the slab
  int64_t slab = 0, fill = 0;       // samples it has room for, samples whose words it holds
  uint64_t *words = nullptr;        // [slab] the words in data order; after the sort, the runs' words
  uint64_t *sorted = nullptr;       // [slab]
  uint32_t *flag = nullptr;         // [slab + 1] run heads, then the new runs
  uint32_t *pos = nullptr;          // [slab + 1] their exclusive scans
  uint32_t *run_start = nullptr;    // [slab + 1]
  uint32_t *info = nullptr;         // [CONN_INFO_WORDS]
  void *tmp = nullptr;              // rocPRIM's own room
  size_t tmp_bytes = 0;
};

static void conn_free_slab(somhip_conn *c) {
  void *p[] = {c->words, c->sorted, c->flag, c->pos, c->run_start};
  for (void *q : p) if (q) (void)hipFree(q);
  c->words = c->sorted = nullptr;
  c->flag = c->pos = c->run_start = nullptr;
  c->slab = c->fill = 0;
}
static void conn_release(somhip_conn *c) {
  conn_free_slab(c);
  for (int i = 0; i < 2; i++) {
    if (c->key[i]) (void)hipFree(c->key[i]);
    if (c->count[i]) (void)hipFree(c->count[i]);
    c->key[i] = c->count[i] = nullptr;
    c->cap[i] = 0;
  }
  if (c->info) (void)hipFree(c->info);
  if (c->tmp) (void)hipFree(c->tmp);
  c->info = nullptr; c->tmp = nullptr; c->tmp_bytes = 0;
  c->n = 0; c->samples = 0; c->units = 0;
  c->e = nullptr;
}
static int check_conn(const somhip_conn *c, bool args, const char *who) {
  if (!c || !args) return fail("%s: null argument", who);
  if (!c->e) return fail("%s: the engine of this pair table was destroyed", who);
  return 0;
}

extern "C" int somhip_conn_create(somhip_engine *e, somhip_conn **out) try {
  if (!e || !out) return fail("somhip_conn_create: null argument");
  HIPCHK(hipSetDevice(e->device));
  somhip_conn *c = new somhip_conn();
  c->e = e;
  e->conns.push_back(c);
  auto fill = [&]() -> int {
    HIPCHK(hipMalloc((void **)&c->info, sizeof(uint32_t) * CONN_INFO_WORDS));
    return 0;
  };
  if (int rc = fill()) { somhip_conn_destroy(c); return rc; }
  *out = c;
  return 0;
} ABI_CATCH(somhip_conn_create)
extern "C" void somhip_conn_destroy(somhip_conn *c) try {
  if (!c) return;
  if (somhip_engine *e = c->e) {                         // an orphan (engine destroyed first) has nothing left on the device
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    conn_release(c);
    e->conns.erase(std::remove(e->conns.begin(), e->conns.end(), c), e->conns.end());
  }
  delete c;
} ABI_CATCH_VOID(somhip_conn_destroy)
extern "C" int somhip_conn_clear(somhip_conn *c) try {
  CHK(check_conn(c, true, "somhip_conn_clear"));
  c->n = 0; c->samples = 0; c->units = 0;                // (the buffers stay)
  return 0;
} ABI_CATCH(somhip_conn_clear)
extern "C" int somhip_conn_size(somhip_conn *c, int64_t *pairs, uint64_t *samples) try {
  CHK(check_conn(c, pairs || samples, "somhip_conn_size"));
  if (pairs) *pairs = c->n;
  if (samples) *samples = c->samples;
  return 0;
} ABI_CATCH(somhip_conn_size)
extern "C" int somhip_conn_read(somhip_conn *c, int64_t first, int64_t n, uint32_t *b1, uint32_t *b2, uint64_t *count) try {
  CHK(check_conn(c, true, "somhip_conn_read"));
  if (first < 0 || n < 0 || first > c->n || n > c->n - first)
    return fail("somhip_conn_read: entries [%lld, +%lld) outside [0, %lld]", (long long)first, (long long)n, (long long)c->n);
  if (n == 0) return 0;
  somhip_engine *e = c->e;
  HIPCHK(hipSetDevice(e->device));
  std::vector<uint64_t> words((size_t)((b1 || b2) ? n : 0));
  if (count) CHK(to_host(e, count, c->count[c->cur] + first, (size_t)n));
  if (!words.empty()) CHK(to_host(e, words.data(), c->key[c->cur] + first, (size_t)n));
  HIPCHK(hipStreamSynchronize(e->stream));
  const uint64_t low = ((uint64_t)1 << c->ubits) - 1;
  for (size_t i = 0; i < words.size(); i++) {
    if (b1) b1[i] = (uint32_t)(words[i] >> c->ubits);
    if (b2) b2[i] = (uint32_t)(words[i] & low);
  }
  return 0;
} ABI_CATCH(somhip_conn_read)

// what somhip_map_connectivity refuses about the table, before anything is launched
static int conn_check_units(const somhip_conn *c, int64_t units, const char *who) {
  if (c->n > 0 && c->units != units)
    return fail("%s: the pair table holds pairs of a codebook of %lld units, this one has %lld (somhip_conn_clear empties it)", who,
                (long long)c->units, (long long)units);
  return 0;
}
static int conn_tmp(somhip_conn *c, size_t bytes) {
  if (c->tmp_bytes >= bytes) return 0;
  if (c->tmp) HIPCHK(hipFree(c->tmp));
  c->tmp = nullptr; c->tmp_bytes = 0;
  HIPCHK(hipMalloc(&c->tmp, bytes));
  c->tmp_bytes = bytes;
  return 0;
}
// opens a run of `count` samples against a codebook of `units` >= 2 units: the slab's room, SOMHIP_CONN_SLAB samples at most
static int conn_begin(somhip_conn *c, int64_t units, int64_t count) {
  if (c->n == 0) { c->units = units; c->ubits = conn_unit_bits((uint64_t)units); }
  c->fill = 0;
  const int64_t want = std::min<int64_t>(count, SOMHIP_CONN_SLAB);
  if (c->slab >= want) return 0;
  conn_free_slab(c);
  const size_t m = (size_t)want;
  HIPCHK(hipMalloc((void **)&c->words, sizeof(uint64_t) * m));
  HIPCHK(hipMalloc((void **)&c->sorted, sizeof(uint64_t) * m));
  HIPCHK(hipMalloc((void **)&c->flag, sizeof(uint32_t) * (m + 1)));
  HIPCHK(hipMalloc((void **)&c->pos, sizeof(uint32_t) * (m + 1)));
  HIPCHK(hipMalloc((void **)&c->run_start, sizeof(uint32_t) * (m + 1)));
  c->slab = want;
  return 0;
}
// room for `want` entries in the buffers the next merge writes
static int conn_reserve_other(somhip_conn *c, int64_t want) {
  const int o = c->cur ^ 1;
  if (c->cap[o] >= want) return 0;
  int64_t cap = std::max(c->cap[o], CONN_FIRST_CAPACITY);
  while (cap < want) cap *= 2;
  if (c->key[o]) HIPCHK(hipFree(c->key[o]));
  if (c->count[o]) HIPCHK(hipFree(c->count[o]));
  c->key[o] = c->count[o] = nullptr; c->cap[o] = 0;
  HIPCHK(hipMalloc((void **)&c->key[o], sizeof(uint64_t) * (size_t)cap));
  HIPCHK(hipMalloc((void **)&c->count[o], sizeof(uint64_t) * (size_t)cap));
  c->cap[o] = cap;
  return 0;
}
static int conn_scan(somhip_conn *c, int kid, const uint32_t *in, uint32_t *out, size_t len) {
  somhip_engine *e = c->e;
  size_t bytes = 0;
  hipError_t er = rocprim::exclusive_scan(nullptr, bytes, in, out, 0u, len, rocprim::plus<uint32_t>(), e->stream);
  if (er != hipSuccess) return fail("map connectivity: the scan's size query failed: %s", hipGetErrorString(er));
  CHK(conn_tmp(c, bytes));
  LaunchTimer t(e, kid);                                                 // (rocPRIM's own launches, on the engine's stream)
  er = rocprim::exclusive_scan(c->tmp, bytes, in, out, 0u, len, rocprim::plus<uint32_t>(), e->stream);
  return er == hipSuccess ? 0 : fail("map connectivity: the scan failed: %s", hipGetErrorString(er));
}

// The slab's words into the table: sort, runs, merge.  Two small copies come back -- the number of runs, which sizes the
// merge and the buffers it writes, and the number of new entries.
static int conn_flush(somhip_conn *c) {
  somhip_engine *e = c->e;
  const uint32_t m = (uint32_t)c->fill;
  c->fill = 0;
  if (m == 0) return 0;
  const auto blocks = [](uint64_t lanes) { return dim3((unsigned)((lanes + CONN_THREADS - 1) / CONN_THREADS)); };
  {
    size_t bytes = 0;
    hipError_t er = rocprim::radix_sort_keys(nullptr, bytes, c->words, c->sorted, (size_t)m, 0u, 2u * c->ubits, e->stream);
    if (er != hipSuccess) return fail("map connectivity: the sort's size query failed: %s", hipGetErrorString(er));
    CHK(conn_tmp(c, bytes));
    LaunchTimer t(e, KID_CONN_SORT);                                     // (rocPRIM's own launches, on the engine's stream)
    er = rocprim::radix_sort_keys(c->tmp, bytes, c->words, c->sorted, (size_t)m, 0u, 2u * c->ubits, e->stream);
    if (er != hipSuccess) return fail("map connectivity: the sort of the slab failed: %s", hipGetErrorString(er));
  }
  CHK(LAUNCH_TIMED(e, KID_CONN_RUNS, k_conn_heads, blocks((uint64_t)m + 1), dim3(CONN_THREADS), 0, c->sorted, m, c->flag));
  CHK(conn_scan(c, KID_CONN_RUNS, c->flag, c->pos, (size_t)m + 1));
  uint64_t *run_key = c->words;                                           // (the unsorted words are done with)
  CHK(LAUNCH_TIMED(e, KID_CONN_RUNS, k_conn_runs, blocks(m), dim3(CONN_THREADS), 0, c->sorted, m, c->pos, run_key, c->run_start, c->info));
  uint32_t info[CONN_INFO_WORDS];
  CHK(to_host_sync(e, info, c->info, CONN_INFO_WORDS));
  const uint32_t runs = info[CONN_INFO_RUNS];
  if (runs == 0) return 0;
  CHK(conn_reserve_other(c, c->n + runs));
  const int o = c->cur ^ 1;
  CHK(LAUNCH_TIMED(e, KID_CONN_MERGE, k_conn_rank, blocks((uint64_t)runs + 1), dim3(CONN_THREADS), 0, run_key, runs, c->key[c->cur], c->n, c->flag));
  CHK(conn_scan(c, KID_CONN_MERGE, c->flag, c->pos, (size_t)runs + 1));
  CHK(LAUNCH_TIMED(e, KID_CONN_MERGE, k_conn_merge, blocks((uint64_t)c->n + runs), dim3(CONN_THREADS), 0, c->key[c->cur], c->count[c->cur], c->n,
      run_key, c->run_start, c->pos, runs, c->key[o], c->count[o]));
  uint32_t added = 0;
  CHK(to_host_sync(e, &added, c->pos + runs, 1));
  c->n += added;
  c->samples += info[CONN_INFO_DEFINED];
  c->cur = o;
  return 0;
}
// the words of one chunk (keys dk[cnt][stride] of the samples from data row f on) behind the slab's; a slab that cannot
// take them goes into the table first
static int conn_take_chunk(somhip_conn *c, const somhip_codebook *cb, const somhip_dataset *ds, int64_t f, int64_t cnt, const uint64_t *dk,
                           int stride) {
  if (c->fill + cnt > c->slab) CHK(conn_flush(c));
  if (cnt > c->slab) return fail("map connectivity: a chunk of %lld samples, the slab holds %lld", (long long)cnt, (long long)c->slab);
  CHK(LAUNCH_TIMED(c->e, KID_CONN_KEYS, k_conn_keys, dim3((unsigned)((cnt + CONN_THREADS - 1) / CONN_THREADS)), dim3(CONN_THREADS), 0, dk, stride,
      ds->d_all_masked, f, ds->n, cnt, cb->v.n, c->ubits, c->words + c->fill));
  c->fill += cnt;
  return 0;
}

// HIP-event totals of the pair passes since somhip_timing_reset, while somhip_timing_enable is on (ids of their own behind
// the published table): [0] k_conn_keys, [1] the sort, [2] the runs (heads, scan, k_conn_runs), [3] the merge (rank, scan,
// k_conn_merge)
extern "C" int somhip_conn_timing(somhip_engine *e, int64_t launches[4], double total_ms[4]) try {
  const int kid[4] = {KID_CONN_KEYS, KID_CONN_SORT, KID_CONN_RUNS, KID_CONN_MERGE};
  return stage_timing(e, "somhip_conn_timing", kid, 4, launches, total_ms);
} ABI_CATCH(somhip_conn_timing)
