/* pak_engine.c -- the single-GPU side of the tools' host library: the engine singleton and the device mirrors, the
 * -selfuncs registry with its per-sample surface, and the epoch-level functions that hand the hot path to
 * libsomhip.so (trainings, scans, initialisations, distance statistics).  Flag names, messages and numerics follow
 * SOM_PAK/LVQ_PAK 3.2 (citations: file:line in hynde/som_lvq_pak). */
#define _GNU_SOURCE
#include "pak_int.h"

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

/* ------------------------------------------------------------------ the HIP back end */
static somhip_engine *g_engine = NULL;
int pak_device = 0;

/* the status of an engine call, after the engine's message when it failed */
static int said(int rc) { if (rc) fprintf(stderr, "%s\n", somhip_last_error()); return rc; }

somhip_engine *pak_engine(void)
{
  if (!g_engine && said(somhip_engine_create(pak_device, &g_engine))) return NULL;
  return g_engine;
}
int pak_engine_is_open(void) { return g_engine != NULL; }
void pak_shutdown(void) { if (g_engine) { somhip_engine_destroy(g_engine); g_engine = NULL; } }

int32_t *pak_first_labels(struct entries *e)
{
  int32_t *l = malloc(sizeof(int32_t) * (e->num_entries + 1));
  for (long r = 0; r < e->num_entries; r++) l[r] = get_entry_label(&e->rows[r]);
  return l;
}

somhip_codebook *pak_mirror_codes(struct entries *codes, int with_labels)
{
  somhip_engine *en = pak_engine();
  if (!en) return NULL;
  somhip_codebook *cb = NULL;
  int32_t *lab = with_labels ? pak_first_labels(codes) : NULL;
  int rc = somhip_codebook_create(en, codes->points, lab, codes->num_entries, codes->dimension, codes->topol,
                                  codes->neigh, codes->xdim, codes->ydim, 0, codes->num_entries, &cb);
  free(lab);
  return said(rc) ? NULL : cb;
}
somhip_dataset *pak_mirror_data(struct entries *data, int with_labels)
{
  somhip_engine *en = pak_engine();
  if (!en) return NULL;
  somhip_dataset *ds = NULL;
  if (data->is_virtual) {
    if (with_labels && pak_materialize(data)) return NULL;
    if (data->is_virtual)
      return said(somhip_dataset_generate(en, data->gen_seed, data->gen_k, data->dimension, 0, data->num_entries, NULL, &ds)) ? NULL : ds;
  }
  int32_t *lab = with_labels ? pak_first_labels(data) : NULL;
  int rc = somhip_dataset_create(en, data->points, data->num_entries, data->dimension,
                                 (const uint8_t *)data->masks, lab, data->weights, data->fixed_xy, &ds);
  free(lab);
  return said(rc) ? NULL : ds;
}

/* the pair a scan works on; both mirrors are always attempted, so each failure gets its message.  0 when both exist */
struct mirrors { somhip_codebook *cb; somhip_dataset *ds; };
static int mirrors_open(struct mirrors *m, struct entries *codes, int code_labels, struct entries *data, int data_labels)
{
  m->cb = pak_mirror_codes(codes, code_labels);
  m->ds = pak_mirror_data(data, data_labels);
  return !(m->cb && m->ds);
}
static void mirrors_close(struct mirrors *m)
{
  if (m->cb) somhip_codebook_destroy(m->cb);
  if (m->ds) somhip_dataset_destroy(m->ds);
}

int pak_check_inputs(struct teach_params *teach, const char *who, int what)
{
  struct entries *data = teach->data;
  if ((what & PAK_CHECK_SOM) && set_som_params(teach)) { fprintf(stderr, "%s: can't set SOM parameters\n", who); return 1; }
  if (!data || data->num_entries <= 0) { fprintf(stderr, "%s: can't get data\n", who); return 1; }
  if ((what & PAK_CHECK_SOM) && data->dimension != teach->codes->dimension) {
    fprintf(stderr, "code dimension (%d) != data dimension (%d)\n", teach->codes->dimension, data->dimension);
    return 1;
  }
  if (what & PAK_CHECK_RANKS) {
    if (data->random_order && data->buffer > 0 && data->buffer < data->num_entries) {
      fprintf(stderr, "%s: -buffer with -rand is not available with -gpus\n", who);
      return 1;
    }
    if (teach->snapshot) fprintf(stderr, "%s: snapshots are not written with -gpus\n", who);
  }
  return 0;
}

/* The per-sample surface of the "hip" row (lvq_pak.h:131-148).  Tools should use the epoch-level functions; these
 * keep per-sample callers of the registry working (balance.c:56, som_rout.c:741,785 dereference dist; the
 * reference's own loops call winner and vector_adapt once per sample).
 *
 * dist / vector_adapt act on ONE host row each -- the host list owns the rows (SURVEY 8b "Ownership") and a
 * PCIe round trip per row would cost a thousand times the arithmetic -- so they are the reference's own
 * expressions on the host rows: vector_dist_euc (lvq_pak.c:291-316) and adapt_vector (lvq_pak.c:339-351),
 * compiled without contraction.  A row written by vector_adapt makes every device mirror stale: the generation
 * counter below makes the next winner call re-upload its codebook. */
static unsigned long host_rows_generation = 0;

static float hip_row_dist(struct data_entry *v1, struct data_entry *v2, int dim)
{
  float sum = 0.0f;
  int masked = 0;
  for (int i = 0; i < dim; i++) {
    if ((v1->mask && v1->mask[i]) || (v2->mask && v2->mask[i])) { masked++; continue; }
    float t = v1->points[i] - v2->points[i];
    sum += t * t;
  }
  if (masked == dim) return -1.0f;                    /* nothing to compare (lvq_pak.c:312-313) */
  return (float)sqrt((double)sum);
}

static void hip_row_adapt(struct data_entry *code, struct data_entry *sample, int dim, float alpha)
{
  for (int i = 0; i < dim; i++) {
    if (sample->mask && sample->mask[i]) continue;    /* only the sample's mask counts (lvq_pak.c:345-346) */
    code->points[i] += alpha * (sample->points[i] - code->points[i]);
  }
  host_rows_generation++;
}

static void hip_drop_mirror(struct entries *codes)
{
  if (codes->userdata) somhip_codebook_destroy(codes->userdata);
  codes->userdata = NULL;
}

static int hip_find_winner(struct entries *codes, struct data_entry *sample, struct winner_info *w, int knn)
{
  somhip_codebook *cb = codes->userdata;
  if (!cb) {
    cb = codes->userdata = pak_mirror_codes(codes, 0);
    codes->drop_mirror = hip_drop_mirror;
    codes->mirror_generation = host_rows_generation;
  }
  if (!cb) return 0;
  if (codes->mirror_generation != host_rows_generation) {       /* rows were adapted on the host since the upload */
    if (said(somhip_codebook_upload(cb, codes->points))) return 0;
    codes->mirror_generation = host_rows_generation;
  }
  somhip_dataset *ds = NULL;
  int32_t idx[8], ret = 0;
  float diff[8];
  if (knn < 1 || knn > 8) return 0;
  if (somhip_dataset_create(pak_engine(), sample->points, 1, codes->dimension, (const uint8_t *)sample->mask,
                            NULL, NULL, NULL, &ds)) return 0;
  int rc = somhip_find_winners(cb, ds, 0, 1, knn, knn > 1 ? SOMHIP_TIE_KNN : SOMHIP_TIE_FIRST, idx, diff, &ret);
  somhip_dataset_destroy(ds);
  if (said(rc)) return 0;
  for (int k = 0; k < knn; k++) {
    w[k].index = idx[k];
    w[k].winner = idx[k] >= 0 ? &codes->rows[idx[k]] : NULL;
    w[k].diff = diff[k];
  }
  return ret;
}

/* the registry (datafile.c:1207-1243).  There is one row, "hip"; the reference's name
 * "default" is accepted as an alias so existing command lines run unchanged.  Unknown names
 * warn and fall back exactly as the reference does. */
static struct vec_functions { const char *name; DIST_FUNCTION *dist; VECTOR_ADAPT *vector_adapt; WINNER_FUNCTION *winner; }
vec_funcs[] = { {"hip", hip_row_dist, hip_row_adapt, hip_find_winner}, {"default", hip_row_dist, hip_row_adapt, hip_find_winner},
                {NULL, NULL, NULL, NULL} };

int set_teach_params(struct teach_params *p, struct entries *codes, struct entries *data, const char *funcname)
{
  struct vec_functions *v = vec_funcs;
  if (funcname)
    for (; v->name; v++) if (strcasecmp(v->name, funcname) == 0) break;
  if (funcname && !v->name) {
    fprintf(stderr, "functions for '%s' not found, using defaults\n", funcname);
    v = vec_funcs;
  }
  p->topol = codes->topol; p->neigh = codes->neigh;
  p->mapdist = NULL; p->neigh_adapt = NULL;
  p->dist = v->dist; p->vector_adapt = v->vector_adapt; p->winner = v->winner;
  p->codes = codes;
  if (data) p->data = data;
  p->snapshot = NULL;
  p->batch = 1;
  return 0;
}
int set_som_params(struct teach_params *p)                   /* som_rout.c:936-947 */
{
  if (p->topol != TOPOL_HEXA && p->topol != TOPOL_RECT) return 1;
  if (p->neigh != NEIGH_BUBBLE && p->neigh != NEIGH_GAUSSIAN) return 1;
  return 0;
}

static int save_snapshot(struct teach_params *teach, long iter)   /* lvq_pak.c:665-774, synchronous form */
{
  char filename[1024], comment[128];
  snprintf(filename, sizeof filename, teach->snapshot->filename, iter);
  snprintf(comment, sizeof comment, "#SNAPSHOT FILE\n#iterations: %ld/%ld\n", iter, teach->length);
  teach->snapshot->counter++;
  return save_entries_wcomments(teach->codes, filename, comment);
}

/* iterations are run in segments that end where the reference would save a snapshot
 * (after iteration le, when le % interval == 0 && le > 0: som_rout.c:650, lvq_rout.c:559) */
static long segment_end(struct teach_params *t, long start)
{
  if (!t->snapshot || t->snapshot->interval <= 0) return t->length;
  const long iv = t->snapshot->interval;
  long next = (start + iv - 1) / iv * iv;             /* smallest le >= start with le % iv == 0 ... */
  if (next == 0) next = iv;                           /* ... and le > 0 (som_rout.c:650) */
  long end = next + 1;
  return end < t->length ? end : t->length;
}

/* The order in which a training run sees the data (datafile.c:237-344, 754-830).  Whole file in
 * memory: the rows as they are (already shuffled once if -rand), cyclically.  -buffer N together
 * with -rand: rows [0,N), [N,2N), ... of the FILE, each buffer shuffled with the running orand()
 * when it is loaded, the file rewound after the last buffer and every run starting at the top.
 * Each buffer becomes a device data set of its own. */
struct feed { struct entries *data, *sub; somhip_dataset *ds; long pos, left, first; int per_buffer, with_labels; };

static int feed_open(struct feed *f, struct entries *data, int with_labels)
{
  memset(f, 0, sizeof *f);
  f->data = data; f->with_labels = with_labels;
  f->per_buffer = data->random_order && data->buffer > 0 && data->buffer < data->num_entries;
  if (!f->per_buffer) { f->ds = pak_mirror_data(data, with_labels); f->left = -1; return f->ds ? 0 : 1; }
  return 0;
}
/* make sure at least one row is available; returns how many consecutive rows can be taken now
 * (*first = index of the next one inside the current device data set), 0 on failure */
static long feed_avail(struct feed *f, long iter, long *first)
{
  if (!f->per_buffer) { *first = iter % f->data->num_entries; return LONG_MAX; }
  if (f->left == 0 || !f->ds) {
    if (f->ds) { somhip_dataset_destroy(f->ds); f->ds = NULL; }
    if (f->sub) { close_entries(f->sub); f->sub = NULL; }
    long n = f->data->num_entries, nb = f->data->buffer < n - f->pos ? f->data->buffer : n - f->pos;
    long *idx = pak_shuffled_rows(f->pos, nb);
    f->sub = pick_rows(f->data, idx, nb);
    free(idx);
    f->ds = pak_mirror_data(f->sub, f->with_labels);
    if (!f->ds) return 0;
    f->left = nb; f->first = 0;
    f->pos = f->pos + nb >= n ? 0 : f->pos + nb;
  }
  *first = f->first;
  return f->left;
}
static void feed_took(struct feed *f, long count) { if (f->per_buffer) { f->left -= count; f->first += count; } }
static void feed_close(struct feed *f)
{
  if (f->ds) somhip_dataset_destroy(f->ds);
  if (f->sub) close_entries(f->sub);
}

/* One training run, segment by segment: as many iterations as the feed has rows for, up to where a snapshot is due;
 * `train` runs them on the engine (0, or non-zero with the engine's last error set), then the snapshot, and the
 * codebook comes back to the host rows at the end.  lvq: the mirrors carry the labels; the two trainings also keep
 * their own snapshot texts and their own (SOM) or no (LVQ) message when the last download fails.  NULL on failure. */
typedef int segment_train(struct teach_params *teach, void *ctx, somhip_codebook *cb, somhip_dataset *ds, long start, long count, long first);

static struct entries *train_in_segments(struct teach_params *teach, const char *who, int lvq, segment_train *train, void *ctx)
{
  struct entries *codes = teach->codes;
  somhip_codebook *cb = pak_mirror_codes(codes, lvq);
  struct feed fd;
  struct entries *ret = NULL;
  if (feed_open(&fd, teach->data, lvq) || !cb) goto done;
  for (long start = 0; start < teach->length;) {
    long first, avail = feed_avail(&fd, start, &first);
    if (avail <= 0) goto done;
    long end = segment_end(teach, start);
    if (end - start > avail) end = start + avail;
    if (train(teach, ctx, cb, fd.ds, start, end - start, first)) { fprintf(stderr, "%s: %s\n", who, somhip_last_error()); goto done; }
    feed_took(&fd, end - start);
    if (teach->snapshot && end - 1 > 0 && (end - 1) % teach->snapshot->interval == 0 && end <= teach->length) {
      if (somhip_codebook_download(cb, codes->points)) goto done;
      if (!lvq) ifverbose(2) fprintf(stderr, "Saving snapshot, %ld iterations\n", end - 1);
      if (save_snapshot(teach, end - 1)) fprintf(stderr, lvq ? "snapshot failed\n" : "snapshot failed, continuing teaching\n");
    }
    start = end;
  }
  if (somhip_codebook_download(cb, codes->points)) { if (!lvq) fprintf(stderr, "%s: %s\n", who, somhip_last_error()); goto done; }
  ret = codes;
done:
  if (cb) somhip_codebook_destroy(cb);
  feed_close(&fd);
  return ret;
}

static int som_segment(struct teach_params *teach, void *ctx, somhip_codebook *cb, somhip_dataset *ds, long start, long count, long first)
{
  somhip_som_params sp = { teach->length, teach->alpha, teach->radius, teach->alpha_type,
                           use_fixed_level, use_weights_level,
                           teach->batch > 1 || teach->batch == SOMHIP_BATCH_AUTO ? teach->batch : 1,   /* -batch auto */
                           start, count, first };
  (void)ctx;
  return somhip_som_train(cb, ds, &sp, NULL, NULL);
}

struct entries *som_training(struct teach_params *teach)     /* som_rout.c:556-671 */
{
  if (pak_check_inputs(teach, "som_training", PAK_CHECK_SOM)) return NULL;
  return train_in_segments(teach, "som_training", 0, som_segment, NULL);
}

/* find_qerror's sum (som_rout.c:705-716) over the winners' squared distances of n rows */
static float qerror_sum(const float *diff, const int32_t *ret, long n)
{
  float qerror = 0.0f;
  for (long i = 0; i < n; i++) {
    if (ret[i] == 0) continue;                          /* ignore empty vectors, :712 */
    qerror += sqrt((double)diff[i]);                    /* float accumulator, :715 */
  }
  return qerror;
}

/* ------------------------------------------------------------------ som_training of a set of maps (vfind)
 * The trials of vfind share data, shape and schedule; on the one-map engine every iteration of every trial is a launch
 * of one workgroup.  A map set trains them all in one launch per chunk of iterations (include/somhip.h, map sets). */
int som_mapset_fits(long n_units, int dim)
{
  int32_t plan[8];
  return n_units > 0 && dim > 0 && somhip_debug_mapset_plan(n_units, dim, 0, plan) == 0 && plan[0] != 0;
}

int som_training_mapset(struct teach_params *teach, float *rows, int n_maps, const struct som_part *parts, int n_parts,
                        struct entries *testdata, float *qerror)
{
  struct entries *codes = teach->codes, *data = teach->data;
  if (pak_check_inputs(teach, "som_training", PAK_CHECK_SOM)) return 1;
  somhip_engine *en = pak_engine();
  if (!en) return 1;
  somhip_mapset *ms = NULL;
  somhip_dataset *ds = NULL, *ts = NULL;
  int32_t *idx = NULL, *ret = NULL;
  float *diff = NULL;
  const char *who = "som_training";                    /* the prefix of an engine error's message */
  int rc = 1;
  if (somhip_mapset_create(en, rows, n_maps, codes->num_entries, codes->dimension, codes->topol, codes->neigh, codes->xdim,
                           codes->ydim, &ms)) goto hip_fail;
  if (!(ds = pak_mirror_data(data, 0))) goto done;
  for (int p = 0; p < n_parts; p++) {
    if (parts[p].length <= 0) continue;                /* (som_training's loop runs no iteration) */
    somhip_som_params sp = { parts[p].length, parts[p].alpha, parts[p].radius, teach->alpha_type, use_fixed_level, use_weights_level,
                             1, 0, parts[p].length, 0 };
    if (somhip_mapset_train(ms, ds, &sp, NULL, NULL)) goto hip_fail;
  }
  if (somhip_mapset_download(ms, 0, n_maps, rows)) goto hip_fail;
  if (qerror) {                                        /* find_qerror (som_rout.c:678-731) of every map */
    const long n = testdata ? testdata->num_entries : 0;
    if (n <= 0) { fprintf(stderr, "find_qerror: can't get data\n"); goto done; }
    if (testdata->dimension != codes->dimension) {
      fprintf(stderr, "code dimension (%d) != data dimension (%d)\n", codes->dimension, testdata->dimension);
      goto done;
    }
    if (!(ts = pak_mirror_data(testdata, 0))) goto done;
    idx = malloc(sizeof(int32_t) * n * n_maps); ret = malloc(sizeof(int32_t) * n * n_maps); diff = malloc(sizeof(float) * n * n_maps);
    who = "find_qerror";
    if (somhip_mapset_winners(ms, ts, 0, n, idx, diff, ret)) goto hip_fail;
    for (int m = 0; m < n_maps; m++) qerror[m] = qerror_sum(diff + m * n, ret + m * n, n);
  }
  rc = 0;
  goto done;
hip_fail:
  fprintf(stderr, "%s: %s\n", who, somhip_last_error());
done:
  free(idx); free(ret); free(diff);
  if (ms) somhip_mapset_destroy(ms);
  if (ds) somhip_dataset_destroy(ds);
  if (ts) somhip_dataset_destroy(ts);
  return rc;
}

/* lvq*_training on one GPU.  Masked data go to the engine with their masks (the exact batched engine takes them); the
 * codes keep their own masks for save_entries. */
struct lvq_run { int kind; float winlen, epsilon, *talpha; };

static int lvq_segment(struct teach_params *teach, void *ctx, somhip_codebook *cb, somhip_dataset *ds, long start, long count, long first)
{
  const struct lvq_run *r = ctx;
  somhip_lvq_params lp = { r->kind, teach->length, teach->alpha, teach->alpha_type, r->winlen, r->epsilon, start, count, first };
  return somhip_lvq_train(cb, ds, &lp, r->talpha, NULL, NULL);
}

static struct entries *lvq_training(struct teach_params *teach, int kind, float winlen, float epsilon,
                                    float *talpha, const char *who)
{
  struct lvq_run r = { kind, winlen, epsilon, talpha };
  if (pak_check_inputs(teach, who, 0)) return NULL;
  return train_in_segments(teach, who, 1, lvq_segment, &r);
}
struct entries *lvq1_training(struct teach_params *t) { return lvq_training(t, SOMHIP_LVQ1, 0, 0, NULL, "lvq1_training"); }
struct entries *lvq2_training(struct teach_params *t, float winlen) { return lvq_training(t, SOMHIP_LVQ2, winlen, 0, NULL, "lvq2_training"); }
struct entries *lvq3_training(struct teach_params *t, float eps, float winlen) { return lvq_training(t, SOMHIP_LVQ3, winlen, eps, NULL, "lvq3_training"); }

struct entries *olvq1_training(struct teach_params *teach, const char *infile, const char *outfile)  /* lvq_rout.c:584-697 */
{
  long noc = teach->codes->num_entries;
  float *talpha = malloc(sizeof(float) * (noc + 1));
  float alpha = teach->alpha;
  if (alpha == 0.0f) {                                        /* :615-622 */
    if (!alpha_read(talpha, noc, infile)) {
      alpha = 0.3f;
      for (long i = 0; i < noc; i++) talpha[i] = alpha;
    }
  } else {
    for (long i = 0; i < noc; i++) talpha[i] = alpha;
  }
  float keep = teach->alpha;
  teach->alpha = alpha;                                       /* the clamp of :671 is the local `alpha` */
  struct entries *r = lvq_training(teach, SOMHIP_OLVQ1, 0, 0, talpha, "olvq1_training");
  teach->alpha = keep;
  if (r) alpha_write(talpha, noc, outfile);                  /* :694 */
  free(talpha);
  return r;
}

int find_all_winners(struct teach_params *teach, int32_t *index, float *diff, int32_t *ret)
{
  struct mirrors m;
  int rc = 1;
  if (!mirrors_open(&m, teach->codes, 0, teach->data, 0))
    rc = said(somhip_find_winners(m.cb, m.ds, 0, teach->data->num_entries, 1, SOMHIP_TIE_FIRST, index, diff, ret));
  mirrors_close(&m);
  return rc;
}

/* an empty map of noc units: header fields, the dense block and the row views into it */
static struct entries *new_codes(int dim, int topol, int neigh, int xdim, int ydim, long noc)
{
  struct entries *codes = calloc(1, sizeof *codes);
  codes->dimension = (short)dim; codes->topol = (short)topol; codes->neigh = (short)neigh;
  codes->xdim = (short)xdim; codes->ydim = (short)ydim; codes->num_entries = noc;
  codes->points = malloc(sizeof(float) * noc * dim);
  codes->rows = calloc(noc, sizeof(struct data_entry));
  for (long k = 0; k < noc; k++) codes->rows[k].points = codes->points + k * dim;
  return codes;
}

/* randinit_codes (som_rout.c:34-162): every component uniform in the bounding box of the data
 * (unmasked components only), orand() drawn unit by unit, component by component. */
struct entries *randinit_codes(struct entries *data, int topol, int neigh, int xdim, int ydim)
{
  int dim = data->dimension;
  long noc = (long)xdim * ydim;
  /* the reference seeds its maximum with FLT_MIN (the smallest positive float), som_rout.c:108-111 */
  float *hi = malloc(sizeof(float) * dim), *lo = malloc(sizeof(float) * dim);
  long *cnt = calloc(dim, sizeof(long));
  for (int i = 0; i < dim; i++) { hi[i] = FLT_MIN; lo[i] = FLT_MAX; }
  if (data->is_virtual) {                              /* the bounding box of a generated source is one pass in HBM */
    somhip_dataset *ds = pak_mirror_data(data, 0);
    int64_t *c64 = malloc(sizeof(int64_t) * dim);
    float *dlo = malloc(sizeof(float) * dim), *dhi = malloc(sizeof(float) * dim);
    if (!ds || somhip_column_minmax(ds, dlo, dhi, c64)) {
      fprintf(stderr, "randinit_codes: %s\n", somhip_last_error());
      free(hi); free(lo); free(cnt); free(c64); free(dlo); free(dhi);
      if (ds) somhip_dataset_destroy(ds);
      return NULL;
    }
    for (int i = 0; i < dim; i++) {
      cnt[i] = (long)c64[i];
      if (cnt[i] > 0) { if (hi[i] < dhi[i]) hi[i] = dhi[i]; if (lo[i] > dlo[i]) lo[i] = dlo[i]; }
    }
    somhip_dataset_destroy(ds);
    free(c64); free(dlo); free(dhi);
  }
  for (long r = 0; !data->is_virtual && r < data->num_entries; r++) {
    struct data_entry *e = &data->rows[r];
    for (int i = 0; i < dim; i++)
      if (!(e->mask && e->mask[i])) {
        cnt[i]++;
        if (hi[i] < e->points[i]) hi[i] = e->points[i];
        if (lo[i] > e->points[i]) lo[i] = e->points[i];
      }
  }
  for (int i = 0; i < dim; i++)
    if (cnt[i] == 0) fprintf(stderr, "randinit_codes: warning! component %d has no data, using 0.0\n", i + 1);
  struct entries *codes = new_codes(dim, topol, neigh, xdim, ydim, noc);
  for (long k = 0; k < noc; k++) {
    for (int i = 0; i < dim; i++)                  /* som_rout.c:140-150 */
      codes->rows[k].points[i] = cnt[i] > 0 ? lo[i] + (hi[i] - lo[i]) * ((float)orand() / 32768.0) : 0.0;
  }
  free(hi); free(lo); free(cnt);
  return codes;
}

/* lininit_codes (som_rout.c:322-429) with find_eigenvectors (:211-320): the map is laid out on the
 * plane spanned by the two principal axes of the data.  The two passes over the data (mean, upper
 * triangle of the centred product sums -- O(n dim^2)) run on the MI355X engine with the reference's
 * fp32 accumulation order; the 10-step two-vector power iteration on the dim x dim matrix is host
 * work, written with the reference's float / double mix so that every rounding falls where it does
 * there. */
static void normalize_f(float *v, int n)              /* som_rout.c:166-174 */
{
  float sum = 0.0;
  for (int j = 0; j < n; j++) sum += v[j] * v[j];
  sum = sqrt(sum);
  for (int j = 0; j < n; j++) v[j] /= sum;
}
static float dotprod_f(const float *v, const float *w, int n)     /* :177-184 */
{
  float sum = 0.0;
  for (int j = 0; j < n; j++) sum += v[j] * w[j];
  return sum;
}
static void gram_schmidt_f(float *v, int n, int e)    /* :187-209 */
{
  float *w = malloc(sizeof(float) * n * e);
  for (int i = 0; i < e; i++) {
    for (int t = 0; t < n; t++) {
      float sum = v[i * n + t];
      for (int j = 0; j < i; j++)
        for (int p = 0; p < n; p++) sum -= w[j * n + t] * w[j * n + p] * v[i * n + p];
      w[i * n + t] = sum;
    }
    normalize_f(w + i * n, n);
  }
  memcpy(v, w, sizeof(float) * n * e);
  free(w);
}

struct entries *lininit_codes(struct entries *data, int topol, int neigh, int xdim, int ydim)
{
  int n = data->dimension;
  long k = data->num_entries, noc = (long)xdim * ydim;
  float *m = malloc(sizeof(float) * n), *r = malloc(sizeof(float) * n * n);
  float *u = malloc(sizeof(float) * 2 * n), *v = malloc(sizeof(float) * 2 * n);
  int64_t *k2 = malloc(sizeof(int64_t) * n);
  float mu[2];
  struct entries *codes = NULL;
  somhip_dataset *ds = pak_mirror_data(data, 0);
  if (!ds) goto fail;
  if (said(somhip_column_sums(ds, m, k2))) goto fail;
  if (k < 3) goto fail;                                 /* :256 */
  for (int i = 0; i < n; i++) m[i] /= k2[i];
  if (said(somhip_centered_products(ds, m, r))) goto fail;
  for (int i = 0; i < n; i++)
    for (int j = i; j < n; j++) r[j * n + i] = r[i * n + j] /= k;
  for (int i = 0; i < 2; i++) {
    for (int j = 0; j < n; j++) u[i * n + j] = orand() / 16384.0 - 1.0;
    normalize_f(u + i * n, n);
    mu[i] = 1.0;
  }
  for (int it = 0; it < 10; it++) {
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < n; j++) v[i * n + j] = mu[i] * dotprod_f(r + j * n, u + i * n, n) + u[i * n + j];
    gram_schmidt_f(v, n, 2);
    float sum = 0.0;                                    /* not reset between the two vectors (:300-306) */
    for (int i = 0; i < 2; i++) {
      for (int j = 0; j < n; j++) sum += fabs(v[i * n + j] / dotprod_f(r + j * n, v + i * n, n));
      mu[i] = sum / n;
    }
    memcpy(u, v, sizeof(float) * 2 * n);
  }
  if (mu[0] == 0.0 || mu[1] == 0.0) goto fail;
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < n; j++) u[i * n + j] /= sqrt(mu[i]);

  codes = new_codes(n, topol, neigh, xdim, ydim, noc);
  for (long index = 0; index < noc; index++) {          /* :405-421 */
    float xf = 4.0 * (float)(index % xdim) / (xdim - 1.0) - 2.0;
    float yf = 4.0 * (float)(index / xdim) / (ydim - 1.0) - 2.0;
    float *pt = codes->rows[index].points;
    for (int i = 0; i < n; i++) pt[i] = m[i] + xf * u[i] + yf * u[n + i];
  }
fail:
  if (!codes) fprintf(stderr, "lininit_codes: Can't find eigenvectors\n");
  if (ds) somhip_dataset_destroy(ds);
  free(m); free(r); free(u); free(v); free(k2);
  return codes;
}

/* k nearest codes of every data row (find_winner_knn, lvq_pak.c:152-221; knn = 1 is
 * find_winner_euc): index/diff [n][knn], nearest first, ties in the reference's order.
 * Masked data rows (`x`) go to the GPU with their masks; the codes' own masks play no part
 * (lvq_pak.c:179-186), and a row with every component masked gets index -2 (no neighbour). */
int find_all_knn(struct entries *codes, struct entries *data, int knn, int32_t *index, float *diff)
{
  if (knn < 1) knn = 1;
  if (knn > 8) { fprintf(stderr, "this engine finds at most 8 nearest neighbours (-knn %d)\n", knn); return 1; }
  struct mirrors m;
  int rc = 1;
  if (!mirrors_open(&m, codes, 0, data, 0))
    rc = said(somhip_find_winners(m.cb, m.ds, 0, data->num_entries, knn, knn >= 2 ? SOMHIP_TIE_KNN : SOMHIP_TIE_FIRST,
                                  index, diff, NULL));
  mirrors_close(&m);
  return rc;
}

/* The class vote of every data row's knn nearest codes (1 <= knn <= SOMHIP_KNN_MAX), formed on the engine behind the
 * search find_all_knn would run (somhip_knn_vote): arrays of data->num_entries.  found = neighbours found; label / freq =
 * head of the hit list after add_hit of their first labels, nearest first (-1 / 0 with no neighbour); own = neighbours
 * with the data row's own first label.  freq, own and found may be NULL.  0, or 1 after a message. */
int knn_vote_all(struct entries *codes, struct entries *data, int knn, int32_t *label, int32_t *freq, int32_t *own,
                 int32_t *found)
{
  if (knn < 1) knn = 1;
  if (knn > SOMHIP_KNN_MAX) { fprintf(stderr, "this engine finds at most %d nearest neighbours (-knn %d)\n", SOMHIP_KNN_MAX, knn); return 1; }
  struct mirrors m;
  int rc = 1;
  if (!mirrors_open(&m, codes, 1, data, own != NULL))                  /* the rows' own labels: only `own` reads them */
    rc = said(somhip_knn_vote(m.cb, m.ds, 0, data->num_entries, knn, label, freq, own, found));
  mirrors_close(&m);
  return rc;
}

/* correct_by_knn (lvq_rout.c:38-78) for every row of `data` against `data` itself: the majority
 * label (head of the hit list built nearest-first) equals the row's own first label. */
unsigned char *knn_correct_all(struct entries *data, int knn)
{
  long n = data->num_entries;
  if (knn < 1) knn = 1;
  int32_t *label = malloc(sizeof(int32_t) * (n + 1)), *found = malloc(sizeof(int32_t) * (n + 1));
  unsigned char *ok = calloc(n, 1);
  if (knn_vote_all(data, data, knn, label, NULL, NULL, found)) { free(label); free(found); free(ok); return NULL; }
  for (long r = 0; r < n; r++) {
    if (found[r] < knn) { fprintf(stderr, "correct_by_knn: can't find winners\n"); ok[r] = 1; }   /* -1 is "true" at :182 */
    else ok[r] = label[r] == get_entry_label(&data->rows[r]);
  }
  free(label); free(found);
  return ok;
}

float find_qerror(struct teach_params *teach)                 /* som_rout.c:678-731 */
{
  if (set_som_params(teach)) { fprintf(stderr, "find_qerror: can't set SOM parameters\n"); return -1; }
  long n = teach->data->num_entries;
  if (n <= 0) { fprintf(stderr, "find_qerror: can't get data\n"); return -1.0f; }
  int32_t *idx = malloc(sizeof(int32_t) * n), *ret = malloc(sizeof(int32_t) * n);
  float *diff = malloc(sizeof(float) * n);
  const float qerror = find_all_winners(teach, idx, diff, ret) ? -1.0f : qerror_sum(diff, ret, n);
  free(idx); free(ret); free(diff);
  return qerror;
}

int find_map_quality(struct teach_params *teach, long buffer, int want_pairs, float distortion_radius, struct map_quality *q)
{
  memset(q, 0, sizeof *q);
  if (set_som_params(teach)) { fprintf(stderr, "find_map_quality: can't set SOM parameters\n"); return 1; }
  const long n = teach->data->num_entries, noc = teach->codes->num_entries;
  if (n <= 0) { fprintf(stderr, "find_map_quality: can't get data\n"); return 1; }
  if (buffer <= 0 || buffer > n) buffer = n;
  q->hits = calloc(noc + 1, sizeof *q->hits);
  q->qsum = calloc(noc + 1, sizeof *q->qsum);
  struct mirrors m;
  somhip_conn *conn = NULL;
  somhip_distortion *dist = NULL;
  int rc = mirrors_open(&m, teach->codes, 0, teach->data, 0);
  if (!rc && want_pairs) rc = said(somhip_conn_create(pak_engine(), &conn));
  if (!rc && distortion_radius >= 0.0f) rc = said(somhip_distortion_create(m.cb, &dist));
  for (long first = 0; !rc && first < n; first += buffer) {      /* hits, qsum and the float chain go from buffer to buffer, */
    somhip_quality_totals t;                                      /* and one pair table takes the pairs of them all */
    const long count = buffer < n - first ? buffer : n - first;
    rc = said(conn ? somhip_map_connectivity(m.cb, m.ds, first, count, conn, q->hits, q->qsum, q->qerror, &t)
                   : somhip_map_quality(m.cb, m.ds, first, count, q->hits, q->qsum, q->qerror, &t));
    if (rc) break;
    q->qerror = t.qerror;
    q->searched += t.searched; q->topo_defined += t.topo_defined; q->topo_errors += t.topo_errors;
    if (dist) rc = said(somhip_distortion_accumulate(dist, m.cb, m.ds, first, count));   /* the chains go from buffer to buffer too */
  }
  if (!rc && dist) {
    somhip_distortion_totals dt;
    q->unit_energy = calloc(noc + 1, sizeof *q->unit_energy);
    rc = said(somhip_distortion_evaluate(dist, m.cb, distortion_radius, q->unit_energy, &dt));
    if (!rc) { q->energy = dt.energy; q->scale = dt.scale; q->distortion_samples = dt.samples; }
  }
  if (!rc && conn) {
    int64_t pairs = 0;
    rc = said(somhip_conn_size(conn, &pairs, NULL));
    if (!rc) {
      q->n_pairs = (long)pairs;
      q->b1 = calloc(pairs + 1, sizeof *q->b1);
      q->b2 = calloc(pairs + 1, sizeof *q->b2);
      q->pair_count = calloc(pairs + 1, sizeof *q->pair_count);
      rc = said(somhip_conn_read(conn, 0, pairs, q->b1, q->b2, q->pair_count));
    }
  }
  if (conn) somhip_conn_destroy(conn);
  if (dist) somhip_distortion_destroy(dist);
  mirrors_close(&m);
  if (rc) free_map_quality(q);
  return rc;
}
void free_map_quality(struct map_quality *q)
{
  free(q->hits); free(q->qsum); free(q->b1); free(q->b2); free(q->pair_count); free(q->unit_energy);
  q->hits = NULL; q->qsum = NULL; q->b1 = q->b2 = NULL; q->pair_count = NULL; q->n_pairs = 0; q->unit_energy = NULL;
}

/* the rows [first, first + count) of data as a device data set of their own, with the rows' first labels or without:
 * uploaded, or -- a gen: source without labels -- generated in place (labels are host rows', so they materialise it) */
somhip_dataset *pak_mirror_rows(struct entries *data, long first, long count, int with_labels)
{
  somhip_engine *en = pak_engine();
  if (!en) return NULL;
  if (with_labels && pak_materialize(data)) return NULL;
  somhip_dataset *ds = NULL;
  const long dim = data->dimension;
  if (data->is_virtual) return said(somhip_dataset_generate(en, data->gen_seed, data->gen_k, (int)dim, first, count, NULL, &ds)) ? NULL : ds;
  int32_t *lab = with_labels ? malloc(sizeof(int32_t) * (count + 1)) : NULL;
  for (long r = 0; lab && r < count; r++) lab[r] = get_entry_label(&data->rows[first + r]);
  int rc = somhip_dataset_create(en, data->points + first * dim, count, (int)dim,
                                 data->masks ? (const uint8_t *)data->masks + first * dim : NULL, lab, NULL, NULL, &ds);
  free(lab);
  return said(rc) ? NULL : ds;
}

/* how a batch training over the whole data opens: who's "can't get data", then both mirrors, with labels or without */
static int batch_open(struct teach_params *teach, const char *who, int with_labels, struct mirrors *m)
{
  m->cb = NULL; m->ds = NULL;
  return pak_check_inputs(teach, who, 0) || mirrors_open(m, teach->codes, with_labels, teach->data, with_labels);
}

static int batchmap_training(struct teach_params *teach, long epochs, long buffer, float *qerror, int missing)
{
  if (set_som_params(teach)) { fprintf(stderr, "som_batchmap_training: can't set SOM parameters\n"); return 1; }
  struct mirrors m = {NULL, NULL};
  int rc;
  if (buffer <= 0) {
    rc = batch_open(teach, "som_batchmap_training", 0, &m);
    if (!rc) {
      somhip_batchmap_params p = {epochs, teach->radius, 0, epochs, 0, teach->data->num_entries};
      rc = said(missing ? somhip_som_batchmap_missing(m.cb, m.ds, &p, qerror) : somhip_som_batchmap(m.cb, m.ds, &p, qerror)) ||
           said(somhip_codebook_download(m.cb, teach->codes->points));
    }
    mirrors_close(&m);
    return rc;
  }
  if (pak_check_inputs(teach, "som_batchmap_training", 0)) return 1;
  /* the epoch over pieces: the sums' chains go on from piece to piece, so any cut gives the bits of one call */
  const long n = teach->data->num_entries, ngroups = (teach->codes->num_entries + 63) / 64;
  rc = !(m.cb = pak_mirror_codes(teach->codes, 0));
  for (long t = 0; !rc && t < epochs; t++) {
    const float r = pak_linear_radius(teach->radius, epochs, t);   /* the engine's r_t */
    rc = said(missing ? somhip_batchmap_missing_begin(m.cb) : somhip_batchmap_begin(m.cb));
    for (long first = 0; !rc && first < n; first += buffer) {
      const long c = buffer < n - first ? buffer : n - first;
      somhip_dataset *piece = pak_mirror_rows(teach->data, first, c, 0);
      rc = !piece || said(missing ? somhip_batchmap_missing_accumulate(m.cb, piece, 0, c, qerror != NULL)
                                  : somhip_batchmap_accumulate(m.cb, piece, 0, c, qerror != NULL));
      if (piece) somhip_dataset_destroy(piece);
    }
    if (!rc) rc = said(missing ? somhip_batchmap_missing_finish(m.cb, r, 0, ngroups, qerror ? qerror + t : NULL)
                               : somhip_batchmap_finish(m.cb, r, 0, ngroups, qerror ? qerror + t : NULL));
  }
  if (!rc) rc = said(somhip_batchmap_end(m.cb)) || said(somhip_codebook_download(m.cb, teach->codes->points));   /* (either form's state) */
  mirrors_close(&m);
  return rc;
}
int som_batchmap_training(struct teach_params *teach, long epochs, long buffer, float *qerror)
{
  return batchmap_training(teach, epochs, buffer, qerror, 0);
}
int som_batchmap_missing_training(struct teach_params *teach, long epochs, long buffer, float *qerror)
{
  return batchmap_training(teach, epochs, buffer, qerror, 1);
}

int glvq_training(struct teach_params *teach, long epochs, float sigmoid_beta, double *cost, int64_t *correct)
{
  struct mirrors m;
  int rc = batch_open(teach, "glvq_training", 1, &m);
  if (!rc) {
    somhip_glvq_params p = {epochs, 0, epochs, 0, teach->data->num_entries, teach->alpha, sigmoid_beta};
    rc = said(somhip_glvq_train(m.cb, m.ds, &p, cost, correct)) || said(somhip_codebook_download(m.cb, teach->codes->points));
  }
  mirrors_close(&m);
  return rc;
}

int glvq_training_buffered(struct teach_params *teach, long epochs, long buffer, float sigmoid_beta, double *cost, int64_t *correct)
{
  if (pak_check_inputs(teach, "glvq_training", 0)) return 1;
  if (buffer < 1) { fprintf(stderr, "glvq_training: buffer %ld < 1\n", buffer); return 1; }
  /* the epoch over pieces, as in batchmap_training */
  const long n = teach->data->num_entries;
  somhip_codebook *cb = pak_mirror_codes(teach->codes, 1);
  int rc = !cb;
  for (long t = 0; !rc && t < epochs; t++) {
    const float alpha_t = pak_linear_rate(teach->alpha, epochs, t);   /* the engine's alpha_t */
    rc = said(somhip_glvq_begin(cb));
    for (long first = 0; !rc && first < n; first += buffer) {
      const long c = buffer < n - first ? buffer : n - first;
      somhip_dataset *piece = pak_mirror_rows(teach->data, first, c, 1);
      rc = !piece || said(somhip_glvq_accumulate(cb, piece, 0, c, sigmoid_beta));
      if (piece) somhip_dataset_destroy(piece);
    }
    if (!rc) rc = said(somhip_glvq_finish(cb, alpha_t, cost ? cost + t : NULL, correct ? correct + t : NULL, NULL));
  }
  if (!rc) rc = said(somhip_glvq_end(cb)) || said(somhip_codebook_download(cb, teach->codes->points));
  if (cb) somhip_codebook_destroy(cb);
  return rc;
}

int rslvq_training(struct teach_params *teach, long epochs, float sigma2, double *cost, int64_t *correct, double *final_cost,
                   int64_t *final_correct, double *pown)
{
  const long n = teach->data->num_entries;
  struct mirrors m;
  int rc = batch_open(teach, "rslvq_training", 1, &m);
  if (!rc && epochs > 0) {
    somhip_rslvq_params p = {epochs, 0, epochs, 0, n, teach->alpha, sigma2};
    rc = said(somhip_rslvq_train(m.cb, m.ds, &p, cost, correct)) || said(somhip_codebook_download(m.cb, teach->codes->points));
  }
  if (!rc) rc = said(somhip_rslvq_search(m.cb, m.ds, 0, n, sigma2, final_cost, final_correct, pown));   /* the state it ends with */
  mirrors_close(&m);
  return rc;
}

/* The state a GRLVQ or GMLVQ run ends with, from one more search's d+ / i+ (d, i) and d- / i- (d + n, i + n) over the n
 * rows, the terms in double here: the cost and the count of correctly classified rows */
static void final_figures(const float *d, const int32_t *i, long n, float sigmoid_beta, double *final_cost, int64_t *final_correct)
{
  double chain = 0.0;
  int64_t right = 0;
  for (long s = 0; s < n; s++) {
    const double dp = (double)d[s], dm = (double)d[n + s], D = dp + dm;
    const double mu = D == 0.0 ? 0.0 : (dp - dm) / D;
    chain += sigmoid_beta != 0.0f ? 1.0 / (1.0 + exp(-(double)sigmoid_beta * mu)) : mu;
    right += d[s] < d[n + s] || (d[s] == d[n + s] && i[s] < i[n + s]);
  }
  *final_cost = chain / (double)n;
  *final_correct = right;
}

int grlvq_training(struct teach_params *teach, long epochs, float sigmoid_beta, float eps, float *lambda, double *cost, int64_t *correct,
                   double *final_cost, int64_t *final_correct)
{
  const long n = teach->data->num_entries;
  struct mirrors m;
  int rc = batch_open(teach, "grlvq_training", 1, &m);
  if (!rc && epochs > 0) {
    somhip_grlvq_params p = {epochs, 0, epochs, 0, n, teach->alpha, sigmoid_beta, eps};
    rc = said(somhip_grlvq_train(m.cb, m.ds, &p, lambda, cost, correct)) || said(somhip_codebook_download(m.cb, teach->codes->points));
  }
  if (!rc) {
    float *d = malloc(sizeof(float) * 2 * (size_t)n);
    int32_t *i = malloc(sizeof(int32_t) * 2 * (size_t)n);
    rc = said(somhip_grlvq_search(m.cb, m.ds, 0, n, lambda, d, i, d + n, i + n));
    if (!rc) final_figures(d, i, n, sigmoid_beta, final_cost, final_correct);
    free(d);
    free(i);
  }
  mirrors_close(&m);
  return rc;
}

int gmlvq_training(struct teach_params *teach, long epochs, float sigmoid_beta, float eps, float *omega, int rank, double *cost,
                   int64_t *correct, double *final_cost, int64_t *final_correct, float *projected)
{
  const long n = teach->data->num_entries;
  struct mirrors m;
  int rc = batch_open(teach, "gmlvq_training", 1, &m);
  if (!rc && epochs > 0) {
    somhip_gmlvq_params p = {epochs, 0, epochs, 0, n, teach->alpha, sigmoid_beta, eps, rank};
    rc = said(somhip_gmlvq_train(m.cb, m.ds, &p, omega, cost, correct)) || said(somhip_codebook_download(m.cb, teach->codes->points));
  }
  if (!rc) {
    float *d = malloc(sizeof(float) * 2 * (size_t)n);
    int32_t *i = malloc(sizeof(int32_t) * 2 * (size_t)n);
    rc = said(somhip_gmlvq_search(m.cb, m.ds, 0, n, omega, rank, d, i, d + n, i + n));
    if (!rc) final_figures(d, i, n, sigmoid_beta, final_cost, final_correct);
    free(d);
    free(i);
  }
  if (!rc && projected) rc = said(somhip_gmlvq_project(m.cb, m.ds, 0, n, omega, rank, projected));
  mirrors_close(&m);
  return rc;
}

int ng_training(struct teach_params *teach, long epochs, double lambda0, double lambda_end, long ranks, struct ng_line *line)
{
  somhip_ng_params p = {epochs, lambda0, lambda_end, ranks, 0, epochs, 0, teach->data->num_entries};
  struct mirrors m;
  int rc = batch_open(teach, "ng_training", 0, &m);
  float *qerror = line ? calloc((size_t)epochs, sizeof *qerror) : NULL;
  if (!rc) rc = said(somhip_ng_train(m.cb, m.ds, &p, qerror)) || said(somhip_codebook_download(m.cb, teach->codes->points));
  for (long t = 0; !rc && line && t < epochs; t++) {
    double w[256];
    int32_t k = 0;
    rc = said(somhip_debug_ng_schedule(&p, teach->codes->num_entries, t, &line[t].lambda, &k, w));
    line[t].ranks = (int)k;
    line[t].qerror = qerror[t];
  }
  mirrors_close(&m);
  free(qerror);
  return rc;
}

int ng_training_dense(struct teach_params *teach, long epochs, double lambda0, double lambda_end, struct ng_line *line)
{
  const long units = teach->codes->num_entries;
  somhip_ng_params p = {epochs, lambda0, lambda_end, 0, 0, epochs, 0, teach->data->num_entries};
  struct mirrors m;
  int rc = batch_open(teach, "ng_training_dense", 0, &m);
  float *qerror = line ? calloc((size_t)epochs, sizeof *qerror) : NULL;
  double *w = line ? malloc(sizeof *w * (size_t)(units > 0 ? units : 1)) : NULL;
  if (!rc) rc = said(somhip_ng_train_dense(m.cb, m.ds, &p, qerror)) || said(somhip_codebook_download(m.cb, teach->codes->points));
  for (long t = 0; !rc && line && t < epochs; t++) {
    rc = said(somhip_debug_ng_dense_schedule(&p, units, t, &line[t].lambda, w));
    line[t].ranks = (int)units;
    line[t].qerror = qerror[t];
  }
  mirrors_close(&m);
  free(w);
  free(qerror);
  return rc;
}

float find_qerror2(struct teach_params *teach)                /* som_rout.c:823-885 */
{
  if (set_som_params(teach)) { fprintf(stderr, "find_qerror2: can't set SOM parameters\n"); return -1; }
  long n = teach->data->num_entries;
  if (n <= 0) { fprintf(stderr, "find_qerror2: can't get data\n"); return -1.0f; }
  ifverbose(3) fprintf(stderr, "qmode 1, %s neighbourhood\n", teach->codes->neigh == NEIGH_GAUSSIAN ? "gaussian" : "bubble");
  float *q = malloc(sizeof(float) * n);
  int32_t *ret = malloc(sizeof(int32_t) * n);
  struct mirrors m;
  float qerror = -1.0f;
  if (!mirrors_open(&m, teach->codes, 0, teach->data, 0) && !said(somhip_qerror2(m.cb, m.ds, teach->radius, 0, n, q, ret))) {
    qerror = 0.0f;
    for (long i = 0; i < n; i++)
      if (ret[i]) qerror += q[i];                             /* ignore empty vectors, :858; float sum :864 */
  }
  mirrors_close(&m);
  free(q); free(ret);
  return qerror;
}

/* ------------------------------------------------------------------ within-class distance statistics */
static int cmp_float(const void *a, const void *b)          /* compar, lvq_rout.c:373-380 */
{
  float x = *(const float *)a, y = *(const float *)b;
  return x < y ? -1 : x > y ? 1 : 0;
}

void free_mindists(struct mindists *md)
{
  if (md) { free(md->cls); free(md->noe); free(md->dists); free(md->devs); free(md); }
}

/* index of `label` among the classes of md, or -1 */
static long mindists_class(const struct mindists *md, long label)
{
  for (long i = 0; i < md->num_classes; i++) if (md->cls[i] == label) return i;
  return -1;
}

/* med_distances, lvq_rout.c:384-491: per class (add_hit's order: most frequent first), the median -- meds[not / 2] of the
 * sorted values -- over its entries of the distance to the nearest LATER entry of the same class; 0 for a class in which
 * no entry has a later one.  The nearest-neighbour search is the engine's (somhip_class_nearest_later: the reference's
 * sums bit for bit); what is left here is one root per entry and the sort.  NULL after a message on failure. */
struct mindists *med_distances(struct entries *codes)
{
  struct mindists *md = calloc(1, sizeof *md);
  struct hitlist *classes = new_hitlist();
  const long n = codes->num_entries;
  for (long r = 0; r < n; r++) add_hit(classes, get_entry_label(&codes->rows[r]));
  const long nol = classes->entries;
  md->num_classes = nol;
  md->cls = calloc(nol + 1, sizeof(long)); md->noe = calloc(nol + 1, sizeof(long)); md->dists = calloc(nol + 1, sizeof(float));
  for (long i = 0; i < nol; i++) { md->cls[i] = classes->label[i]; md->noe[i] = classes->freq[i]; }
  free_hitlist(classes);
  if (n == 0) return md;

  float *min_sq = malloc(sizeof(float) * n), *meds = malloc(sizeof(float) * n);
  int32_t *state = malloc(sizeof(int32_t) * n);
  somhip_dataset *ds = pak_mirror_data(codes, 1);
  int rc = 1;
  if (ds) {
    rc = said(somhip_class_nearest_later(ds, min_sq, state));
    somhip_dataset_destroy(ds);
  }
  if (!rc) {
    long *start = calloc(nol + 1, sizeof(long)), *not = calloc(nol + 1, sizeof(long));
    for (long i = 1; i < nol; i++) start[i] = start[i - 1] + md->noe[i - 1];
    for (long r = 0; r < n; r++) {                          /* every class's values, in row order */
      if (state[r] == 0) continue;                          /* `fou` stayed 0: no later entry of the class */
      const long i = mindists_class(md, get_entry_label(&codes->rows[r]));
      float dissf;
      if (state[r] == 2) dissf = -1;                        /* vector_dist_euc's "nothing to compare" beats every distance */
      else if (isinf(min_sq[r])) dissf = FLT_MAX;           /* no distance passed `dist < dissf` */
      else dissf = sqrt(min_sq[r]);
      meds[start[i] + not[i]++] = dissf;
    }
    for (long i = 0; i < nol; i++)
      if (not[i] > 0) { qsort(meds + start[i], not[i], sizeof(float), cmp_float); md->dists[i] = meds[start[i] + not[i] / 2]; }
    free(start); free(not);
  }
  free(min_sq); free(meds); free(state);
  if (rc) { free_mindists(md); return NULL; }
  return md;
}

/* deviations, lvq_rout.c:929-1004, on the host (one pass of n x dim additions): per class of md the fp32 column sums of
 * `data` in row order, the row's masked components skipped, divided by md's class count -- the codebook's when md comes
 * from a codebook, as the reference does it -- then per row devdist (lvq_rout.c:918-927: all components, no mask) added
 * per class in row order, and sqrt(devs / noe).  The reference indexes past its arrays for a label md has no class for;
 * here that is refused: returns 1 after a message that names the label. */
int deviations(struct entries *data, struct mindists *md)
{
  const int dim = data->dimension;
  const long nol = md->num_classes;
  free(md->devs);
  md->devs = calloc(nol + 1, sizeof(float));
  float *avers = calloc((size_t)(nol + 1) * dim, sizeof(float));
  long *cls_of = malloc(sizeof(long) * (data->num_entries + 1));
  for (long r = 0; r < data->num_entries; r++) {
    const int label = get_entry_label(&data->rows[r]);
    if ((cls_of[r] = mindists_class(md, label)) < 0) {
      const char *name = find_conv_to_lab(label);
      fprintf(stderr, "deviations: label '%s' of the data (entry %ld) is carried by no codebook entry\n", name ? name : "", r + 1);
      free(avers); free(cls_of);
      return 1;
    }
    const struct data_entry *e = &data->rows[r];
    float *a = avers + cls_of[r] * dim;
    for (int j = 0; j < dim; j++)
      if (!(e->mask && e->mask[j])) a[j] += e->points[j];
  }
  for (long i = 0; i < nol; i++)
    for (int j = 0; j < dim; j++) avers[i * dim + j] /= md->noe[i];
  for (long r = 0; r < data->num_entries; r++) {
    const float *v1 = data->rows[r].points, *v2 = avers + cls_of[r] * dim;
    float d = 0.0;
    for (int j = 0; j < dim; j++) { float diff = v1[j] - v2[j]; d += diff * diff; }
    md->devs[cls_of[r]] += d;
  }
  for (long i = 0; i < nol; i++) md->devs[i] = sqrt(md->devs[i] / md->noe[i]);
  free(avers); free(cls_of);
  return 0;
}
