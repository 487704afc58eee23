// host_comm.inc -- collectives for a C host that runs one process per GPU (include/somhip.h, "multi-GPU host")
// (included by somhip.hip: one translation unit, shared static helpers)
//
// RCCL is called directly: ncclAllReduce(keys, ncclUint64, ncclMin) on the engine's own HIP stream is the X1
// exchange of SURVEY 8e, so scan -> all-reduce -> update stay stream-ordered with no host synchronisation.
// librccl.so is opened on first use (dlopen): a process that never creates a communicator -- the C tools on one
// GPU, bench.py (which reaches RCCL through torch.distributed) -- never loads it.
//
// A second transport, plain host sockets in a star around rank 0, exists for rehearsals where several ranks share
// one GPU (RCCL refuses duplicate devices) and for the save-time gather of a host array; every operation of it
// synchronises the stream and stages through the host.
#include <cerrno>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <sys/socket.h>
#include <unistd.h>

namespace {
struct RcclApi {
  void *so = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Broadcast)(const void *, void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;

int rccl_load() {
  if (g_rccl.so) return 0;
  const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void *so = nullptr;
  for (const char *n : names) if ((so = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
  if (!so) return fail("RCCL: cannot open librccl.so (%s)", dlerror());
#define SYM(field, name)                                                                     \
  *reinterpret_cast<void **>(&g_rccl.field) = dlsym(so, name);                                \
  if (!g_rccl.field) return fail("RCCL: librccl.so has no %s", name)
  SYM(GetUniqueId, "ncclGetUniqueId");
  SYM(CommInitRank, "ncclCommInitRank");
  SYM(CommDestroy, "ncclCommDestroy");
  SYM(AllReduce, "ncclAllReduce");
  SYM(AllGather, "ncclAllGather");
  SYM(Broadcast, "ncclBroadcast");
  SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
  g_rccl.so = so;
  return 0;
}
#define NCCLCHK(expr)                                                                                  \
  do {                                                                                                 \
    ncclResult_t r_ = (expr);                                                                          \
    if (r_ != ncclSuccess) return fail("%s: %s (%s:%d)", #expr, g_rccl.GetErrorString(r_), __FILE__, __LINE__); \
  } while (0)

// whole transfers; an interrupted call (a profiler's or timer's signal) is repeated, and a peer that has exited is an
// error return -- MSG_NOSIGNAL: no SIGPIPE -- so that the rank leaves through fail() with its message and clean-up
int write_all(int fd, const void *buf, size_t n) {
  const char *p = static_cast<const char *>(buf);
  while (n) {
    ssize_t k = send(fd, p, n, MSG_NOSIGNAL);
    if (k < 0 && errno == ENOTSOCK) k = write(fd, p, n);       // (a pipe handed in by a test)
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return 1;
    p += k; n -= (size_t)k;
  }
  return 0;
}
int read_all(int fd, void *buf, size_t n) {
  char *p = static_cast<char *>(buf);
  while (n) {
    ssize_t k = read(fd, p, n);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return 1;
    p += k; n -= (size_t)k;
  }
  return 0;
}
}  // namespace

struct somhip_comm {
  somhip_engine *e = nullptr;
  int rank = 0, world = 1;
  ncclComm_t nccl = nullptr;          // RCCL transport
  std::vector<int> fds;               // socket transport: rank 0 holds world-1 descriptors (peer r at [r-1]), the others one
  std::vector<uint8_t> stage, stage2;
};

extern "C" int somhip_comm_unique_id(void *id128) try {
  if (!id128) return fail("somhip_comm_unique_id: null argument");
  CHK(rccl_load());
  ncclUniqueId id;
  NCCLCHK(g_rccl.GetUniqueId(&id));
  memcpy(id128, &id, sizeof id);
  return 0;
} ABI_CATCH(somhip_comm_unique_id)

extern "C" int somhip_comm_create(somhip_engine *e, const void *id128, int rank, int world, somhip_comm **out) try {
  if (!e || !id128 || !out) return fail("somhip_comm_create: null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail("somhip_comm_create: rank %d of %d", rank, world);
  CHK(rccl_load());
  HIPCHK(hipSetDevice(e->device));
  somhip_comm *c = new somhip_comm();
  c->e = e; c->rank = rank; c->world = world;
  ncclUniqueId id;
  memcpy(&id, id128, sizeof id);
  ncclResult_t r = g_rccl.CommInitRank(&c->nccl, world, id, rank);
  if (r != ncclSuccess) { delete c; return fail("ncclCommInitRank: %s", g_rccl.GetErrorString(r)); }
  *out = c;
  return 0;
} ABI_CATCH(somhip_comm_create)

extern "C" int somhip_comm_create_sockets(somhip_engine *e, int rank, int world, const int *fds, somhip_comm **out) try {
  if (!e || !out || (world > 1 && !fds)) return fail("somhip_comm_create_sockets: null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail("somhip_comm_create_sockets: rank %d of %d", rank, world);
  somhip_comm *c = new somhip_comm();
  c->e = e; c->rank = rank; c->world = world;
  if (world > 1) c->fds.assign(fds, fds + (rank == 0 ? world - 1 : 1));
  *out = c;
  return 0;
} ABI_CATCH(somhip_comm_create_sockets)

extern "C" void somhip_comm_destroy(somhip_comm *c) try {
  if (!c) return;
  if (c->nccl) (void)g_rccl.CommDestroy(c->nccl);
  delete c;
} ABI_CATCH_VOID(somhip_comm_destroy)

// star all-reduce / all-gather of host buffers (socket transport, and host arrays at save time)
template <class Reduce>
static int star_allreduce(somhip_comm *c, void *host, size_t bytes, Reduce reduce) {
  if (c->world == 1) return 0;
  if (c->rank == 0) {
    c->stage2.resize(bytes);
    for (int r = 1; r < c->world; r++) {
      if (read_all(c->fds[(size_t)r - 1], c->stage2.data(), bytes)) return fail("somhip_comm: rank %d went away", r);
      reduce(host, c->stage2.data());
    }
    for (int r = 1; r < c->world; r++) if (write_all(c->fds[(size_t)r - 1], host, bytes)) return fail("somhip_comm: rank %d went away", r);
  } else {
    if (write_all(c->fds[0], host, bytes) || read_all(c->fds[0], host, bytes)) return fail("somhip_comm: rank 0 went away");
  }
  return 0;
}

extern "C" int somhip_comm_allreduce_min_keys(somhip_comm *c, uint64_t *dev_keys, int64_t count) try {
  if (!c || !dev_keys) return fail("somhip_comm_allreduce_min_keys: null argument");
  if (count <= 0) return 0;
  somhip_engine *e = c->e;
  HIPCHK(hipSetDevice(e->device));
  if (c->nccl) {                                         // X1: in place, on the engine's stream, no host synchronisation
    NCCLCHK(g_rccl.AllReduce(dev_keys, dev_keys, (size_t)count, ncclUint64, ncclMin, c->nccl, e->stream));
    return 0;
  }
  c->stage.resize(sizeof(uint64_t) * (size_t)count);
  CHK(to_host_sync(e, c->stage.data(), reinterpret_cast<const uint8_t *>(dev_keys), c->stage.size()));
  CHK(star_allreduce(c, c->stage.data(), c->stage.size(), [count](void *a, const void *b) {
    uint64_t *x = static_cast<uint64_t *>(a);
    const uint64_t *y = static_cast<const uint64_t *>(b);
    for (int64_t i = 0; i < count; i++) x[i] = y[i] < x[i] ? y[i] : x[i];
  }));
  CHK(to_device(e, reinterpret_cast<uint8_t *>(dev_keys), c->stage.data(), c->stage.size()));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_comm_allreduce_min_keys)

extern "C" int somhip_comm_allreduce_min_f32(somhip_comm *c, float *dev_values, int64_t count) try {
  if (!c || !dev_values) return fail("somhip_comm_allreduce_min_f32: null argument");
  if (count <= 0) return 0;
  somhip_engine *e = c->e;
  HIPCHK(hipSetDevice(e->device));
  if (c->nccl) {                                         // the exchanged pre-filter bounds (somhip_shard_winner_*)
    NCCLCHK(g_rccl.AllReduce(dev_values, dev_values, (size_t)count, ncclFloat32, ncclMin, c->nccl, e->stream));
    return 0;
  }
  c->stage.resize(sizeof(float) * (size_t)count);
  CHK(to_host_sync(e, c->stage.data(), reinterpret_cast<const uint8_t *>(dev_values), c->stage.size()));
  CHK(star_allreduce(c, c->stage.data(), c->stage.size(), [count](void *a, const void *b) {
    float *x = static_cast<float *>(a);
    const float *y = static_cast<const float *>(b);
    for (int64_t i = 0; i < count; i++) x[i] = y[i] < x[i] ? y[i] : x[i];
  }));
  CHK(to_device(e, reinterpret_cast<uint8_t *>(dev_values), c->stage.data(), c->stage.size()));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_comm_allreduce_min_f32)

extern "C" int somhip_comm_allreduce_sum_u32(somhip_comm *c, uint32_t *dev_words, int64_t count) try {
  if (!c || !dev_words) return fail("somhip_comm_allreduce_sum_u32: null argument");
  if (count <= 0) return 0;
  somhip_engine *e = c->e;
  HIPCHK(hipSetDevice(e->device));
  if (c->nccl) {
    NCCLCHK(g_rccl.AllReduce(dev_words, dev_words, (size_t)count, ncclUint32, ncclSum, c->nccl, e->stream));
    return 0;
  }
  c->stage.resize(sizeof(uint32_t) * (size_t)count);
  CHK(to_host_sync(e, c->stage.data(), reinterpret_cast<const uint8_t *>(dev_words), c->stage.size()));
  CHK(star_allreduce(c, c->stage.data(), c->stage.size(), [count](void *a, const void *b) {
    uint32_t *x = static_cast<uint32_t *>(a);
    const uint32_t *y = static_cast<const uint32_t *>(b);
    for (int64_t i = 0; i < count; i++) x[i] += y[i];
  }));
  CHK(to_device(e, reinterpret_cast<uint8_t *>(dev_words), c->stage.data(), c->stage.size()));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_comm_allreduce_sum_u32)

extern "C" int somhip_comm_allgather(somhip_comm *c, const void *dev_send, void *dev_recv, int64_t bytes_per_rank) try {
  if (!c || !dev_send || !dev_recv) return fail("somhip_comm_allgather: null argument");
  if (bytes_per_rank <= 0) return 0;
  somhip_engine *e = c->e;
  HIPCHK(hipSetDevice(e->device));
  if (c->nccl) {
    NCCLCHK(g_rccl.AllGather(dev_send, dev_recv, (size_t)bytes_per_rank, ncclUint8, c->nccl, e->stream));
    return 0;
  }
  const size_t per = (size_t)bytes_per_rank;
  c->stage.resize(per * (size_t)c->world);
  CHK(to_host_sync(e, c->stage.data() + per * (size_t)c->rank, static_cast<const uint8_t *>(dev_send), per));
  if (c->world > 1) {
    if (c->rank == 0) {
      for (int r = 1; r < c->world; r++) if (read_all(c->fds[(size_t)r - 1], c->stage.data() + per * (size_t)r, per)) return fail("somhip_comm: rank %d went away", r);
      for (int r = 1; r < c->world; r++) if (write_all(c->fds[(size_t)r - 1], c->stage.data(), c->stage.size())) return fail("somhip_comm: rank %d went away", r);
    } else {
      if (write_all(c->fds[0], c->stage.data() + per * (size_t)c->rank, per) || read_all(c->fds[0], c->stage.data(), c->stage.size()))
        return fail("somhip_comm: rank 0 went away");
    }
  }
  CHK(to_device(e, static_cast<uint8_t *>(dev_recv), c->stage.data(), c->stage.size()));
  HIPCHK(hipStreamSynchronize(e->stream));
  return 0;
} ABI_CATCH(somhip_comm_allgather)

// dev_buf of rank `root` to every rank's dev_buf (the batch map's state going from rank to rank, host_batchmap.inc)
extern "C" int somhip_comm_broadcast(somhip_comm *c, void *dev_buf, int64_t bytes, int root) try {
  if (!c || !dev_buf) return fail("somhip_comm_broadcast: null argument");
  if (root < 0 || root >= c->world) return fail("somhip_comm_broadcast: root %d of %d ranks", root, c->world);
  if (bytes <= 0) return 0;
  somhip_engine *e = c->e;
  HIPCHK(hipSetDevice(e->device));
  if (c->nccl) {
    NCCLCHK(g_rccl.Broadcast(dev_buf, dev_buf, (size_t)bytes, ncclUint8, root, c->nccl, e->stream));
    return 0;
  }
  if (c->world == 1) return 0;
  // the star: the root's bytes reach rank 0, which passes them to every other rank
  c->stage.resize((size_t)bytes);
  if (c->rank == root) CHK(to_host_sync(e, c->stage.data(), static_cast<const uint8_t *>(dev_buf), c->stage.size()));
  if (c->rank == 0) {
    if (root != 0 && read_all(c->fds[(size_t)root - 1], c->stage.data(), c->stage.size())) return fail("somhip_comm: rank %d went away", root);
    for (int r = 1; r < c->world; r++)
      if (r != root && write_all(c->fds[(size_t)r - 1], c->stage.data(), c->stage.size())) return fail("somhip_comm: rank %d went away", r);
  } else if (c->rank == root ? write_all(c->fds[0], c->stage.data(), c->stage.size()) : read_all(c->fds[0], c->stage.data(), c->stage.size()))
    return fail("somhip_comm: rank 0 went away");
  if (c->rank != root) {
    CHK(to_device(e, static_cast<uint8_t *>(dev_buf), c->stage.data(), c->stage.size()));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  return 0;
} ABI_CATCH(somhip_comm_broadcast)
