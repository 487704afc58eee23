/* pak_ranks.c -- the multi-process side of the tools' host library: the fork/socketpair rank launcher with its kill
 * logic, and the drivers of `vsom -gpus G`, `lvqtrain -gpus G`, `bsom -gpus G` and `glvq -gpus G` that run in every rank. */
#define _GNU_SOURCE
#include "pak_int.h"

#include <errno.h>
#include <signal.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

/* ------------------------------------------------------------------ som_training on G GPUs (vsom -gpus G)
 * One process per GPU: the parent -- which has parsed the arguments and read the files, and has not
 * touched a GPU -- forks G ranks; rank r takes device r % (visible GPUs), holds every G-th 8x8-unit patch of the map
 * (somhip_codebook_create_interleaved; contiguous row blocks when a map side is not a multiple of 8) and the whole
 * data set.  Per mini-batch: somhip_batch_winner_keys on its shard (or somhip_shard_winner_begin / refine / finish with
 * the pre-filter's bounds MIN-reduced between them) -> somhip_comm_allreduce_min_keys (RCCL
 * ncclAllReduce(ncclUint64, ncclMin) on the engine's stream; the ranks get the communicator id from rank 0 over a
 * socketpair the parent made) -> somhip_som_batch_update of its own rows.  The codebook comes together only at the end
 * (X3), on rank 0, which returns it for saving.  When the ranks outnumber the GPUs (a rehearsal on one GPU: RCCL
 * refuses duplicate devices) or SOMHIP_COMM=sockets, the keys travel over the same sockets instead. */

/* whole transfers over the ranks' sockets: interrupted calls are repeated; a peer that went away is an error return
 * (MSG_NOSIGNAL: no SIGPIPE), so that the caller's own clean-up and message are what happens */
static int sock_write(int fd, const void *b, size_t n)
{
  const char *p = b;
  while (n) {
    ssize_t k = send(fd, p, n, MSG_NOSIGNAL);
    if (k < 0 && errno == ENOTSOCK) k = write(fd, p, n);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return 1;
    p += k; n -= (size_t)k;
  }
  return 0;
}
static int sock_read(int fd, void *b, size_t n)
{
  char *p = b;
  while (n) {
    ssize_t k = read(fd, p, n);
    if (k < 0 && errno == EINTR) continue;
    if (k <= 0) return 1;
    p += k; n -= (size_t)k;
  }
  return 0;
}

/* The ranks' communicator: RCCL when every rank has a GPU of its own (or SOMHIP_COMM=rccl), with the id made by rank 0
 * and passed over the sockets; the sockets themselves otherwise.  0, 1 with the engine's last error set, or -1 when a
 * peer went away (no message). */
static int rank_comm_open(somhip_engine *en, int rank, int world, int ndev, int *fds, somhip_comm **comm, int *use_rccl)
{
  const char *force = getenv("SOMHIP_COMM");
  *use_rccl = force ? strcmp(force, "rccl") == 0 : ndev >= world;
  if (!*use_rccl) return somhip_comm_create_sockets(en, rank, world, fds, comm) != 0;
  char id[128];
  if (rank == 0) {
    if (somhip_comm_unique_id(id)) return 1;
    for (int r = 1; r < world; r++) if (sock_write(fds[r - 1], id, sizeof id)) return -1;
  } else if (sock_read(fds[0], id, sizeof id)) return -1;
  return somhip_comm_create(en, id, rank, world, comm) != 0;
}

/* the contiguous block [r0, r1) of n rows that belongs to `rank` of `world` (empty for ranks past the end) */
static void rank_block(long n, int world, int rank, long *r0, long *r1)
{
  const long per = (n + world - 1) / world;
  *r0 = rank * per < n ? rank * per : n;
  *r1 = *r0 + per < n ? *r0 + per : n;
}

/* what one rank does; fds: rank 0 has world-1 descriptors (peer r at [r-1]), every other rank one (to rank 0) */
static int som_training_rank(struct teach_params *teach, int rank, int world, int *fds)
{
  struct entries *codes = teach->codes, *data = teach->data;
  const long n = codes->num_entries, dim = codes->dimension, L = teach->length;
  const int auto_b = teach->batch == SOMHIP_BATCH_AUTO;     /* -batch auto: the engine's own batch boundaries */
  const long B = auto_b ? 32768 : teach->batch > 1 ? teach->batch : 4096;
  int ndev = 0, rc = 1;
  somhip_comm *comm = NULL;
  somhip_codebook *cb = NULL;
  somhip_dataset *ds = NULL;
  void *dkeys = NULL, *dbound = NULL, *dflag = NULL;
  int64_t *units = NULL, n_local = 0;
  float *mine = NULL;
  if (pak_rank_device(rank) < 0 || somhip_device_count(&ndev)) return 1;
  somhip_engine *en = pak_engine();
  if (!en) return 1;
  int use_rccl;
  const int no_comm = rank_comm_open(en, rank, world, ndev, fds, &comm, &use_rccl);
  if (no_comm > 0) goto hip_fail;
  if (no_comm) goto done;
  ifverbose(2) fprintf(stderr, "rank %d/%d on GPU %d, keys by %s\n", rank, world, pak_device, use_rccl ? "RCCL" : "host sockets");

  /* this rank's units and rows */
  const int interleaved = codes->xdim % 8 == 0 && codes->ydim % 8 == 0;
  if (interleaved) {
    if (somhip_shard_units(codes->xdim, codes->ydim, rank, world, NULL, &n_local)) goto hip_fail;
    units = malloc(sizeof(int64_t) * (n_local + 1));
    if (somhip_shard_units(codes->xdim, codes->ydim, rank, world, units, &n_local)) goto hip_fail;
  } else {
    long r0, r1;
    rank_block(n, world, rank, &r0, &r1);
    n_local = r1 - r0;
    units = malloc(sizeof(int64_t) * (n_local + 1));
    for (long j = 0; j < n_local; j++) units[j] = r0 + j;
  }
  if (n_local <= 0) { fprintf(stderr, "som_training: more ranks (%d) than the map can be cut into\n", world); goto done; }
  mine = malloc(sizeof(float) * n_local * dim);
  for (long j = 0; j < n_local; j++) memcpy(mine + j * dim, codes->points + units[j] * dim, sizeof(float) * dim);
  if (interleaved ? somhip_codebook_create_interleaved(en, mine, n_local, (int)dim, codes->topol, codes->neigh, codes->xdim, codes->ydim, rank, world, &cb)
                  : somhip_codebook_create(en, mine, NULL, n_local, (int)dim, codes->topol, codes->neigh, codes->xdim, codes->ydim, units[0], n, &cb)) goto hip_fail;
  if (!(ds = pak_mirror_data(data, 0))) goto done;
  if (somhip_device_alloc(en, 8 * B, &dkeys) || somhip_device_alloc(en, 4 * B, &dbound) || somhip_device_alloc(en, 16, &dflag)) goto hip_fail;
  long exch_c = -1;
  int exch_ok = 0;

  somhip_som_params sp = { L, teach->alpha, teach->radius, teach->alpha_type, use_fixed_level, use_weights_level, B, 0, 0, 0 };
  for (long it0 = 0; it0 < L;) {                       /* batches aligned to the schedule, as somhip_som_train cuts them */
    long c = B - it0 % B < L - it0 ? B - it0 % B : L - it0;
    const long first = it0 % data->num_entries;
    if (auto_b) {
      int64_t bs, bl;
      if (somhip_som_auto_batch(&sp, n, codes->topol, codes->neigh, it0, &bs, &bl)) goto hip_fail;
      c = (long)(bs + bl - it0);
    }
    if (c != exch_c) {                                 /* every rank has to take the same path: the answers are summed once per batch length */
      /* (the exchange pays from 8 ranks on -- tools/shard_rehearsal.py; SOMHIP_SHARD_EXCHANGE=1 asks for it with fewer) */
      uint32_t f = (world >= 8 || (world > 1 && getenv("SOMHIP_SHARD_EXCHANGE"))) && somhip_shard_exchange_available(cb, ds, c) ? 1u : 0u;
      if (somhip_copy_to_device(en, dflag, &f, sizeof f) || somhip_comm_allreduce_sum_u32(comm, dflag, 1) ||
          somhip_copy_to_host(en, &f, dflag, sizeof f)) goto hip_fail;
      exch_ok = f == (uint32_t)world;
      if (exch_ok && exch_c < 0 && rank == 0) ifverbose(2) fprintf(stderr, "winner search: pre-filter bounds exchanged between the %d ranks\n", world);
      exch_c = c;
    }
    /* the winner search of the whole map: with the pre-filter's bounds going round between its levels every rank
     * re-ranks only what one GPU holding the whole map would (somhip.h, somhip_shard_winner_*) */
    if (exch_ok ? (somhip_shard_winner_begin(cb, ds, first, c, dkeys, dbound) || somhip_comm_allreduce_min_f32(comm, dbound, c) ||
                   somhip_shard_winner_refine(cb, ds, first, c, dbound) || somhip_comm_allreduce_min_f32(comm, dbound, c) ||
                   somhip_shard_winner_finish(cb, ds, first, c, dbound, dkeys))
                : somhip_batch_winner_keys(cb, ds, first, c, dkeys)) goto hip_fail;
    if (somhip_comm_allreduce_min_keys(comm, dkeys, c) || somhip_som_batch_update(cb, ds, &sp, it0, c, first, dkeys)) goto hip_fail;
    it0 += c;
  }
  if (somhip_codebook_download(cb, mine)) goto hip_fail;
  /* X3: every rank's rows, with their unit indices, to rank 0 */
  if (rank == 0) {
    for (long j = 0; j < n_local; j++) memcpy(codes->points + units[j] * dim, mine + j * dim, sizeof(float) * dim);
    for (int r = 1; r < world; r++) {
      int64_t cnt;
      if (sock_read(fds[r - 1], &cnt, sizeof cnt)) goto done;
      int64_t *u = malloc(sizeof(int64_t) * (cnt + 1));
      float *rows = malloc(sizeof(float) * (cnt + 1) * dim);
      const int bad = sock_read(fds[r - 1], u, sizeof(int64_t) * cnt) || sock_read(fds[r - 1], rows, sizeof(float) * cnt * dim);
      for (long j = 0; !bad && j < cnt; j++) memcpy(codes->points + u[j] * dim, rows + j * dim, sizeof(float) * dim);
      free(u); free(rows);
      if (bad) goto done;
    }
  } else if (sock_write(fds[0], &n_local, sizeof n_local) || sock_write(fds[0], units, sizeof(int64_t) * n_local) ||
             sock_write(fds[0], mine, sizeof(float) * n_local * dim)) goto done;
  rc = 0;
  goto done;
hip_fail:
  fprintf(stderr, "som_training (rank %d): %s\n", rank, somhip_last_error());
done:
  if (dkeys) somhip_device_free(en, dkeys);
  if (dbound) somhip_device_free(en, dbound);
  if (dflag) somhip_device_free(en, dflag);
  if (ds) somhip_dataset_destroy(ds);
  if (cb) somhip_codebook_destroy(cb);
  if (comm) somhip_comm_destroy(comm);
  free(units); free(mine);
  return rc;
}

/* Ends the ranks still alive: SIGTERM, a grace period, SIGKILL, and reaps every one of them (a rank that sits in a
 * collective whose peer is gone -- ncclAllReduce / hipStreamSynchronize -- never returns by itself). */
static void ranks_kill_rest(pid_t *pid, int world)
{
  int alive = 0;
  for (int r = 0; r < world; r++) if (pid[r] > 0) { kill(pid[r], SIGTERM); alive++; }
  for (int tick = 0; alive && tick < 50; tick++) {           /* up to 5 s */
    for (int r = 0; r < world; r++)
      if (pid[r] > 0 && waitpid(pid[r], NULL, WNOHANG) == pid[r]) { pid[r] = 0; alive--; }
    if (alive) { struct timespec ts = {0, 100000000}; nanosleep(&ts, NULL); }
  }
  for (int r = 0; r < world; r++)
    if (pid[r] > 0) { kill(pid[r], SIGKILL); waitpid(pid[r], NULL, 0); pid[r] = 0; }
}

/* One process per GPU: forks `world` ranks of the calling process -- which has read its files and has NOT touched a GPU
 * yet -- and runs rank_main(rank, world, fds, arg) in each; fds: rank 0 gets world-1 socket descriptors (peer r at
 * [r-1]), every other rank one (to rank 0).  Rank r uses device r % (visible GPUs) (pak_rank_device).  Returns 0 when
 * every rank returned 0.  The ranks are reaped in the order in which they end; the first one that fails (non-zero exit
 * or a signal) -- or a fork() that fails half way -- ends the others (ranks_kill_rest) and the call returns 1: no rank
 * is left behind in a collective, no orphan keeps a GPU.  Children are only ever started fresh or killed, never
 * re-executed. */
int pak_run_ranks(int world, int (*rank_main)(int rank, int world, int *fds, void *arg), void *arg)
{
  if (pak_engine_is_open()) { fprintf(stderr, "the ranks must be started before this process uses a GPU\n"); return 1; }
  if (world < 1 || world > 64) { fprintf(stderr, "-gpus %d?\n", world); return 1; }
  int (*sv)[2] = malloc(sizeof(int[2]) * (world > 1 ? world - 1 : 1));
  for (int r = 1; r < world; r++)
    if (socketpair(AF_UNIX, SOCK_STREAM, 0, sv[r - 1])) {
      perror("socketpair");
      for (int q = 1; q < r; q++) { close(sv[q - 1][0]); close(sv[q - 1][1]); }
      free(sv);
      return 1;
    }
  pid_t *pid = calloc((size_t)world, sizeof(pid_t));
  fflush(NULL);
  int bad = 0;
  for (int r = 0; r < world && !bad; r++) {
    pid[r] = fork();
    if (pid[r] < 0) { perror("fork"); pid[r] = 0; bad = 1; break; }
    if (pid[r] == 0) {
      signal(SIGPIPE, SIG_IGN);      /* a peer that went away is an error return of the write (host_comm.inc), not a signal */
      int *fds = malloc(sizeof(int) * (world > 1 ? world - 1 : 1));
      for (int q = 1; q < world; q++) {
        if (r == 0) { fds[q - 1] = sv[q - 1][0]; close(sv[q - 1][1]); }
        else if (q == r) { fds[0] = sv[q - 1][1]; close(sv[q - 1][0]); }
        else { close(sv[q - 1][0]); close(sv[q - 1][1]); }
      }
      const int rc = rank_main(r, world, fds, arg);
      pak_shutdown();
      fflush(NULL);
      _exit(rc ? 1 : 0);
    }
  }
  for (int r = 1; r < world; r++) { close(sv[r - 1][0]); close(sv[r - 1][1]); }
  int left = 0;
  for (int r = 0; r < world; r++) if (pid[r] > 0) left++;
  while (!bad && left > 0) {
    int st = 0;
    const pid_t w = waitpid(-1, &st, 0);
    if (w < 0) { if (errno == EINTR) continue; bad = 1; break; }
    int r = 0;
    while (r < world && pid[r] != w) r++;
    if (r == world) continue;                                  /* some other child of the host program */
    pid[r] = 0; left--;
    if (!WIFEXITED(st) || WEXITSTATUS(st) != 0) {
      if (WIFSIGNALED(st)) fprintf(stderr, "rank %d ended by signal %d; stopping the other ranks\n", r, WTERMSIG(st));
      else fprintf(stderr, "rank %d failed; stopping the other ranks\n", r);
      bad = 1;
    }
  }
  if (bad) ranks_kill_rest(pid, world);
  free(sv); free(pid);
  return bad;
}
int pak_rank_device(int rank)
{
  int ndev = 0;
  if (somhip_device_count(&ndev) || ndev < 1) { fprintf(stderr, "%s\n", somhip_last_error()); return -1; }
  pak_device = rank % ndev;
  return pak_device;
}
int pak_sock_write(int fd, const void *b, size_t n) { return sock_write(fd, b, n); }
int pak_sock_read(int fd, void *b, size_t n) { return sock_read(fd, b, n); }

struct som_multi { struct teach_params *teach; int (*after)(struct teach_params *, void *); void *arg; };
static int som_multi_rank(int rank, int world, int *fds, void *p)
{
  struct som_multi *m = p;
  int rc = som_training_rank(m->teach, rank, world, fds);
  if (rc == 0 && rank == 0 && m->after) rc = m->after(m->teach, m->arg);
  return rc;
}
/* vsom -gpus G: the ranks train the sharded map; rank 0 also runs after(teach, arg) -- the tool's "save the codebook" */
int som_training_multi(struct teach_params *teach, int gpus, int (*after)(struct teach_params *, void *), void *arg)
{
  if (pak_check_inputs(teach, "som_training", PAK_CHECK_SOM | PAK_CHECK_RANKS)) return 1;
  struct som_multi m = { teach, after, arg };
  return pak_run_ranks(gpus, som_multi_rank, &m);
}

/* ------------------------------------------------------------------ lvq*_training on G GPUs (lvqtrain -gpus G)
 * The codebook is cut into contiguous row blocks, one per rank; every rank holds the data.  Per batch of <= 1024
 * iterations (include/somhip.h, "lvq*_training over a ROW-SHARDED codebook"): each rank's 8 nearest rows per sample ->
 * all-gather + merge -> labels / rates / rows of the listed candidates the rank owns -> all-reduce(SUM) as integers ->
 * every rank walks the batch (same decisions everywhere) and commits the rows it owns.  Exactly the online result.
 * Masked data: every rank's data set carries the masks (mirror_data), so the scan, the walk and its components use them.
 * Collectives: RCCL when every rank has its own GPU, the parent's socketpairs otherwise (somhip_comm). */
struct lvq_multi {
  struct teach_params *teach; int kind; float winlen, epsilon, clamp; float *talpha;
  int (*after)(struct teach_params *, void *); void *arg;
};

static int lvq_training_rank(int rank, int world, int *fds, void *pp)
{
  struct lvq_multi *m = pp;
  struct teach_params *teach = m->teach;
  struct entries *codes = teach->codes, *data = teach->data;
  const long n = codes->num_entries, dim = codes->dimension, L = teach->length;
  long r0, r1;
  rank_block(n, world, rank, &r0, &r1);
  const long nl = r1 - r0;
  const int knn = m->kind >= SOMHIP_LVQ2 ? 2 : 1, XR = 4, BMAX = 1024;
  const long d4 = (dim + 3) / 4;
  int ndev = 0, rc = 1;
  somhip_comm *comm = NULL;
  somhip_codebook *cb = NULL;
  somhip_dataset *ds = NULL;
  void *dloc = NULL, *dall = NULL, *dkeys = NULL, *dlab = NULL, *dta = NULL, *drows = NULL;
  float *mine = NULL;
  if (nl <= 0) { fprintf(stderr, "lvq training: more ranks (%d) than code vectors\n", world); return 1; }
  if (pak_rank_device(rank) < 0 || somhip_device_count(&ndev)) return 1;
  somhip_engine *en = pak_engine();
  if (!en) return 1;
  int use_rccl;
  const int no_comm = rank_comm_open(en, rank, world, ndev, fds, &comm, &use_rccl);
  if (no_comm > 0) goto hip_fail;
  if (no_comm) goto done;

  int32_t *lab = pak_first_labels(codes);
  if (somhip_codebook_create(en, codes->points + r0 * dim, lab + r0, nl, (int)dim, TOPOL_LVQ, 0, 0, 0, r0, n, &cb)) { free(lab); goto hip_fail; }
  free(lab);
  if (m->kind == SOMHIP_OLVQ1 && somhip_lvq_rates_upload(cb, m->talpha + r0)) goto hip_fail;
  if (!(ds = pak_mirror_data(data, 1))) goto done;
  if (somhip_device_alloc(en, 8 * 8 * BMAX, &dloc) || somhip_device_alloc(en, (int64_t)8 * 8 * BMAX * world, &dall) ||
      somhip_device_alloc(en, 8 * 8 * BMAX, &dkeys) || somhip_device_alloc(en, 4 * 8 * BMAX, &dlab) ||
      somhip_device_alloc(en, 4 * 8 * BMAX, &dta) || somhip_device_alloc(en, (int64_t)BMAX * XR * d4 * 16, &drows)) goto hip_fail;

  somhip_lvq_params lp = { m->kind, L, m->clamp, teach->alpha_type, m->winlen, m->epsilon, 0, 0, 0 };
  long B = 256;
  for (long it0 = 0; it0 < L;) {
    const long c = B < L - it0 ? B : L - it0, first = it0 % data->num_entries;
    int64_t done = 0;
    if (somhip_batch_topk_keys(cb, ds, first, c, 8, knn == 2 ? SOMHIP_TIE_KNN : SOMHIP_TIE_FIRST, dloc) ||
        somhip_comm_allgather(comm, dloc, dall, 8 * 8 * c) ||
        somhip_merge_topk_keys(en, dall, world, c, 8, dkeys) ||
        somhip_lvq_batch_candidates(cb, c, m->kind, dkeys, XR, dlab, m->kind == SOMHIP_OLVQ1 ? dta : NULL, drows) ||
        somhip_comm_allreduce_sum_u32(comm, dlab, 8 * c) ||
        (m->kind == SOMHIP_OLVQ1 && somhip_comm_allreduce_sum_u32(comm, dta, 8 * c)) ||
        somhip_comm_allreduce_sum_u32(comm, drows, c * XR * d4 * 4) ||
        somhip_lvq_batch_apply(cb, ds, &lp, it0, c, first, dkeys, dlab, m->kind == SOMHIP_OLVQ1 ? dta : NULL, drows, XR, &done, NULL, NULL))
      goto hip_fail;
    if (done <= 0 || done > c) { fprintf(stderr, "lvq training: batch made no progress\n"); goto done; }
    it0 += done;
    B = done == c ? (2 * B < BMAX ? 2 * B : BMAX) : (done + done / 4 + 8 > 32 ? (done + done / 4 + 8 < BMAX ? done + done / 4 + 8 : BMAX) : 32);
  }
  /* X3: every rank's rows (and OLVQ1 rates) to rank 0 */
  mine = malloc(sizeof(float) * nl * (dim + 1));
  if (somhip_codebook_download(cb, mine)) goto hip_fail;
  if (m->kind == SOMHIP_OLVQ1 && somhip_lvq_rates_download(cb, mine + nl * dim)) goto hip_fail;
  if (rank == 0) {
    memcpy(codes->points, mine, sizeof(float) * nl * dim);
    if (m->kind == SOMHIP_OLVQ1) memcpy(m->talpha, mine + nl * dim, sizeof(float) * nl);
    for (int r = 1; r < world; r++) {
      long q0, q1;
      rank_block(n, world, r, &q0, &q1);
      const long nq = q1 - q0;
      float *buf = malloc(sizeof(float) * (nq + 1) * (dim + 1));
      const int bad = sock_read(fds[r - 1], buf, sizeof(float) * nq * (dim + 1));
      if (!bad) {
        memcpy(codes->points + q0 * dim, buf, sizeof(float) * nq * dim);
        if (m->kind == SOMHIP_OLVQ1) memcpy(m->talpha + q0, buf + nq * dim, sizeof(float) * nq);
      }
      free(buf);
      if (bad) goto done;
    }
    rc = m->after ? m->after(teach, m->arg) : 0;
  } else {
    rc = sock_write(fds[0], mine, sizeof(float) * nl * (dim + 1));
  }
  goto done;
hip_fail:
  fprintf(stderr, "lvq training (rank %d): %s\n", rank, somhip_last_error());
done:
  { void *bufs[6] = { dloc, dall, dkeys, dlab, dta, drows }; for (int k = 0; k < 6; k++) if (bufs[k]) somhip_device_free(en, bufs[k]); }
  if (ds) somhip_dataset_destroy(ds);
  if (cb) somhip_codebook_destroy(cb);
  if (comm) somhip_comm_destroy(comm);
  free(mine);
  return rc;
}

/* lvqtrain -gpus G.  talpha: OLVQ1's rates, [noc], filled in by the caller as lvq_rout.c:614-627 does and updated in
 * rank 0's copy before after(teach, arg) runs there (save the codebook, write the .lra file). */
int lvq_training_multi(struct teach_params *teach, int kind, float winlen, float epsilon, float clamp, float *talpha, int gpus,
                       int (*after)(struct teach_params *, void *), void *arg)
{
  if (pak_check_inputs(teach, "lvq training", PAK_CHECK_RANKS)) return 1;
  struct lvq_multi m = { teach, kind, winlen, epsilon, clamp, talpha, after, arg };
  return pak_run_ranks(gpus, lvq_training_rank, &m);
}

/* ------------------------------------------------------------------ the data in row blocks on G GPUs (bsom -gpus G, glvq -gpus G)
 * The DATA is cut into contiguous row blocks, one per rank, with its labels where the trainer reads them; every rank
 * holds the whole codebook.  The trainer's *_ranks call runs the epochs: the winner search of every block at the same
 * time, the ordered sums rank after rank with the state broadcast in between, the same update (the batch map: the combine
 * divided by row groups) on every rank.  Every rank ends with the same codebook and per-epoch figures; rank 0 returns them. */
struct epoch_figures { float *qerror; double *cost; int64_t *correct; };   /* [epochs] each, or NULL */
struct block_multi {
  struct teach_params *teach; long epochs; float beta; const char *who; int with_labels;
  /* the one call that trains over the ranks, on this rank's block of `rows` rows; f: this rank's own arrays */
  int (*train)(const struct block_multi *m, somhip_codebook *cb, somhip_dataset *ds, long rows, somhip_comm *comm, struct epoch_figures *f);
  struct epoch_figures out;              /* the caller's: rank 0 copies into those that are not NULL before after(teach, arg) */
  int (*after)(struct teach_params *, void *); void *arg;
};

static int block_training_rank(int rank, int world, int *fds, void *pp)
{
  struct block_multi *m = pp;
  struct entries *codes = m->teach->codes, *data = m->teach->data;
  const size_t epochs = (size_t)m->epochs;
  long r0, r1;
  rank_block(data->num_entries, world, rank, &r0, &r1);
  int ndev = 0, rc = 1;
  somhip_comm *comm = NULL;
  somhip_codebook *cb = NULL;
  somhip_dataset *ds = NULL;
  /* every rank asks for its figures: the chain goes through all of them */
  struct epoch_figures f = { calloc(epochs + 1, sizeof *f.qerror), calloc(epochs + 1, sizeof *f.cost), calloc(epochs + 1, sizeof *f.correct) };
  somhip_engine *en = pak_rank_device(rank) < 0 || somhip_device_count(&ndev) ? NULL : pak_engine();
  if (!en) goto done;
  int use_rccl;
  const int no_comm = rank_comm_open(en, rank, world, ndev, fds, &comm, &use_rccl);
  if (no_comm > 0) goto hip_fail;
  if (no_comm) goto done;
  ifverbose(2) fprintf(stderr, "rank %d/%d on GPU %d, data rows [%ld, %ld), state by %s\n", rank, world, pak_device, r0, r1,
                       use_rccl ? "RCCL" : "host sockets");
  if (!(cb = pak_mirror_codes(codes, m->with_labels))) goto done;
  if (r1 > r0 && !(ds = pak_mirror_rows(data, r0, r1 - r0, m->with_labels))) goto done;
  if (m->train(m, cb, ds, r1 - r0, comm, &f)) goto hip_fail;
  if (rank == 0) {
    if (somhip_codebook_download(cb, codes->points)) goto hip_fail;
    if (m->out.qerror) memcpy(m->out.qerror, f.qerror, sizeof *f.qerror * epochs);
    if (m->out.cost) memcpy(m->out.cost, f.cost, sizeof *f.cost * epochs);
    if (m->out.correct) memcpy(m->out.correct, f.correct, sizeof *f.correct * epochs);
    rc = m->after ? m->after(m->teach, m->arg) : 0;
  } else rc = 0;
  goto done;
hip_fail:
  fprintf(stderr, "%s (rank %d): %s\n", m->who, rank, somhip_last_error());
done:
  if (ds) somhip_dataset_destroy(ds);
  if (cb) somhip_codebook_destroy(cb);
  if (comm) somhip_comm_destroy(comm);
  free(f.qerror); free(f.cost); free(f.correct);
  return rc;
}

static int batchmap_over_ranks(const struct block_multi *m, somhip_codebook *cb, somhip_dataset *ds, long rows, somhip_comm *comm, struct epoch_figures *f)
{
  somhip_batchmap_params p = { m->epochs, m->teach->radius, 0, m->epochs, 0, rows };
  return somhip_som_batchmap_ranks(cb, ds, &p, comm, f->qerror);
}
int som_batchmap_training_multi(struct teach_params *teach, long epochs, float *qerror, int gpus,
                                int (*after)(struct teach_params *, void *), void *arg)
{
  if (pak_check_inputs(teach, "som_batchmap_training", PAK_CHECK_SOM | PAK_CHECK_RANKS)) return 1;
  struct block_multi m = { teach, epochs, 0.0f, "som_batchmap_training", 0, batchmap_over_ranks, { qerror, NULL, NULL }, after, arg };
  return pak_run_ranks(gpus, block_training_rank, &m);
}

static int glvq_over_ranks(const struct block_multi *m, somhip_codebook *cb, somhip_dataset *ds, long rows, somhip_comm *comm, struct epoch_figures *f)
{
  somhip_glvq_params p = { m->epochs, 0, m->epochs, 0, rows, m->teach->alpha, m->beta };
  return somhip_glvq_train_ranks(cb, ds, &p, comm, f->cost, f->correct);
}
int glvq_training_multi(struct teach_params *teach, long epochs, float sigmoid_beta, double *cost, int64_t *correct, int gpus,
                        int (*after)(struct teach_params *, void *), void *arg)
{
  if (pak_check_inputs(teach, "glvq_training", PAK_CHECK_RANKS)) return 1;
  struct block_multi m = { teach, epochs, sigmoid_beta, "glvq_training", 1, glvq_over_ranks, { NULL, cost, correct }, after, arg };
  return pak_run_ranks(gpus, block_training_rank, &m);
}
