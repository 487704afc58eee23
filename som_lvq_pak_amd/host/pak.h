/* pak.h -- host side of the MI355X SOM/LVQ tools, in C.
 *
 * The command-line tools here (vsom, lvqtrain = lvq1/olvq1/lvq2/lvq3, qerror, accuracy, vcal)
 * keep the flags, file formats and output text of SOM_PAK/LVQ_PAK 3.2 so existing .dat/.cod
 * files and scripts drop in; the hot path goes through the C ABI of libsomhip.so
 * (include/somhip.h).  The plug-in surface keeps the reference's names and meaning
 * (struct teach_params and its function-pointer types, lvq_pak.h:131-148,186-204; registry
 * selected with -selfuncs, datafile.c:1207-1243) so code written against that interface still
 * reads the same -- but the storage behind it is dense (one float block per file, rows are
 * views), because that is what a GPU mirror wants.
 */
#ifndef PAK_H
#define PAK_H

#include <stdio.h>
#include <stdint.h>
#include "somhip.h"

/* ids as in the reference (lvq_pak.h:209-224) */
#define TOPOL_UNKNOWN 0
#define TOPOL_DATA 1
#define TOPOL_LVQ 2
#define TOPOL_HEXA 3
#define TOPOL_RECT 4
#define NEIGH_UNKNOWN 0
#define NEIGH_BUBBLE 1
#define NEIGH_GAUSSIAN 2
#define ALPHA_UNKNOWN 0
#define ALPHA_LINEAR 1
#define ALPHA_INVERSE_T 2
#define LABEL_EMPTY 0

struct fixpoint { short xfix, yfix; };

/* one row: a view into its file's dense blocks */
struct data_entry {
  float *points;
  int *labels;          /* num_labs label ids */
  short num_labs;
  short weight;
  char *mask;           /* NULL or dim flags, nonzero = ignore component */
  struct fixpoint *fixed;
};

struct entries {
  short dimension, topol, neigh, xdim, ydim;
  long num_entries;
  struct data_entry *rows;      /* [num_entries] views */
  float *points;                /* [num_entries][dimension] */
  char *masks;                  /* NULL if no row has a masked component */
  short *fixed_xy;              /* [num_entries][2], -1 = none (NULL if none at all) */
  short *weights;               /* [num_entries] (NULL if none) */
  int labels_needed;
  long buffer;                  /* > 0 with random_order: -buffer N -rand, rows are presented buffer by buffer, */
  int random_order;             /*   each buffer reshuffled when it is (re)loaded (datafile.c:237-344)            */
  int is_virtual;               /* a `gen:` source kept as its specification: rows exist only on the device */
  unsigned long long gen_seed;  /*   (vsom / qerror / randinit / lininit, see pak_gen_virtual_ok); pak_materialize() */
  int gen_k;                    /*   makes the host rows when something needs them after all                        */
  void *userdata;               /* device mirror handle (as lvq_pak.h:112) */
  void (*drop_mirror)(struct entries *);   /* set by whoever sets userdata (pak_engine.c, per-sample surface): close_entries calls it */
  unsigned long mirror_generation;   /* host-row generation the mirror was uploaded at (pak_engine.c, per-sample surface) */
};

struct winner_info { long index; struct data_entry *winner; float diff; };

struct teach_params;
typedef void  NEIGH_ADAPT(struct teach_params *, struct data_entry *sample, int bx, int by, float radius, float alpha);
typedef void  VECTOR_ADAPT(struct data_entry *c, struct data_entry *s, int d, float a);
typedef float MAPDIST_FUNCTION(int bx, int by, int tx, int ty);
typedef float DIST_FUNCTION(struct data_entry *v1, struct data_entry *v2, int dim);
typedef int   WINNER_FUNCTION(struct entries *codes, struct data_entry *sample, struct winner_info *w, int knn);
typedef float ALPHA_FUNC(long iter, long length, float alpha);

struct snapshot_info { long interval; char *filename; int counter; };

struct teach_params {
  short topol, neigh, alpha_type;
  MAPDIST_FUNCTION *mapdist;
  DIST_FUNCTION *dist;
  NEIGH_ADAPT *neigh_adapt;
  VECTOR_ADAPT *vector_adapt;
  WINNER_FUNCTION *winner;
  ALPHA_FUNC *alpha_func;
  float radius, alpha;
  long length;
  int knn;
  struct entries *codes, *data;
  struct snapshot_info *snapshot;
  long batch;                   /* new: -batch B (1 = the reference's online schedule) */
};

/* ---- arguments, verbosity (same conventions as lvq_pak.c:583-660) ---- */
#define ALWAYS 1
#define OPTION 0
#define OPTION2 2
char *extract_parameter(int argc, char **argv, const char *param, int when);
long oatoi(const char *s, long def);
float oatof(const char *s, float def);
int global_options(int argc, char **argv);
extern int verbose_level;
#define ifverbose(l) if (verbose_level >= (l))
const char *pak_progname(const char *argv0);

/* ---- labels (1-based ids in order of first appearance; labels.c:75) ---- */
int find_conv_to_ind(const char *str);
const char *find_conv_to_lab(int ind);
int number_of_labels(void);
#define get_entry_label(e) ((e)->num_labs > 0 ? (e)->labels[0] : LABEL_EMPTY)

/* frequency-ordered hit lists (labels.c:370-407): new labels go last, a label moves up while
 * its predecessor has a strictly smaller count */
struct hitlist { long *label, *freq; long entries, cap; };
struct hitlist *new_hitlist(void);
void free_hitlist(struct hitlist *);
long add_hit(struct hitlist *, long label);
long hitlist_label_freq(struct hitlist *, long label);

/* ---- files ---- */
int pak_parse_float(const char *s, float *out);     /* = sscanf(s, "%f", out) > 0, fast path for plain decimals */
struct entries *open_entries(const char *name, int labels_needed, int skip_empty);
int save_entries_wcomments(struct entries *codes, const char *name, const char *comments);
#define save_entries(c, n) save_entries_wcomments((c), (n), NULL)
/* raw fp32 side format ("#!somf32", pak_io.c) -- open_entries reads it transparently, this writes it */
int save_entries_f32(struct entries *c, const char *name);
/* `-din gen:...` without a host copy: tools whose whole use of the data is epoch-level calls of the engine set this
 * before open_entries(); the rows are then generated in HBM by somhip_dataset_generate when the mirror is made (a
 * 10 M x 512 stream is 20 GB the host never allocates, parses or sends over PCIe).  Sources with labels=1, and any
 * later need for host rows (-rand, -buffer), materialise as before. */
extern int pak_gen_virtual_ok;
int pak_materialize(struct entries *e);
/* the seeded Gaussian-mixture stream behind `-din gen:k=..,dim=..,n=..,seed=..[,labels=1]` (pak_io.c) */
uint64_t pak_splitmix64(uint64_t x);
float pak_gen_z(uint64_t seed, uint64_t counter);
void pak_gen_row(uint64_t seed, int k_centres, int dim, long row, float *out, int *centre);
int pak_parse_gen(const char *spec, long *n, int *dim, int *k, uint64_t *seed, int *labels);
int pak_gen_unlabelled(const char *name);          /* 1: a `gen:` source without labels=1 */
void close_entries(struct entries *);
void clear_entry_labels(struct entries *e, long row);
void add_entry_label(struct entries *e, long row, int label);
int alpha_read(float *alpha, long noc, const char *infile);
int alpha_write(float *alpha, long noc, const char *outfile);
void invalidate_alphafile(const char *outfile);

/* ---- RNG + -rand shuffle (lvq_pak.c:459-484, datafile.c:1152-1188) ---- */
void init_random(int seed);
long orand(void);
void randomize_entry_order(struct entries *e);

/* ---- the registry (-selfuncs) and the epoch-level functions behind it ---- */
int set_teach_params(struct teach_params *p, struct entries *codes, struct entries *data, const char *funcname);
int set_som_params(struct teach_params *p);
ALPHA_FUNC linear_alpha, inverse_t_alpha;
ALPHA_FUNC *alpha_func_by_name(const char *name, short *id);
extern int use_fixed_level, use_weights_level;

struct entries *som_training(struct teach_params *teach);
struct entries *lvq1_training(struct teach_params *teach);
struct entries *olvq1_training(struct teach_params *teach, const char *infile, const char *outfile);
struct entries *lvq2_training(struct teach_params *teach, float winlen);
struct entries *lvq3_training(struct teach_params *teach, float epsilon, float winlen);
/* som_training of many maps of one shape at once (a somhip map set; vfind's trials): every map comes out as som_training
 * leaves it, bit for bit.  teach gives the data, the schedule's alpha_type and, through teach->codes, the lattice of ONE
 * such map; rows [n_maps][units][dim] are trained in place through the parts in turn (length, alpha, radius each).
 * qerror, if not NULL, receives find_qerror of every trained map on testdata.  0, or 1 after a message. */
struct som_part { long length; float alpha, radius; };
int som_mapset_fits(long n_units, int dim);         /* 1: maps of this shape can be trained as a set (their image fits on chip) */
int som_training_mapset(struct teach_params *teach, float *rows, int n_maps, const struct som_part *parts, int n_parts,
                        struct entries *testdata, float *qerror);
float find_qerror(struct teach_params *teach);
float find_qerror2(struct teach_params *teach);   /* qerror -qetype 1 (som_rout.c:823) */
/* find_qerror's sum together with the topographic error and the per-unit statistics of the map (somhip_map_quality), the
 * data taken `buffer` rows per engine call (<= 0: at once) with the same result.  hits / qsum: arrays of the codebook's
 * entries.  want_pairs: the same search also counts the samples per ordered pair (best unit, second-best unit)
 * (somhip_map_connectivity, one pair table through all buffers): b1 / b2 / pair_count are the n_pairs pairs with a non-zero
 * count, ascending by (b1, b2).  distortion_radius >= 0: the map's distortion at that radius too (somhip_distortion_*, one
 * state through all buffers, a winner search of its own per buffer): energy, scale, distortion_samples and unit_energy, an
 * array of the codebook's entries; < 0: none.  The arrays are the caller's to free (free_map_quality).  0, or 1 after a
 * message. */
struct map_quality {
  float qerror; long searched, topo_defined, topo_errors; uint32_t *hits; double *qsum;
  long n_pairs; uint32_t *b1, *b2; uint64_t *pair_count;
  double energy, scale; unsigned long long distortion_samples; double *unit_energy;
};
int find_map_quality(struct teach_params *teach, long buffer, int want_pairs, float distortion_radius, struct map_quality *q);
void free_map_quality(struct map_quality *q);
/* Kohonen's batch map (somhip_som_batchmap): `epochs` epochs over all of teach->data from teach->radius down to 1, the
 * lattice and neighbourhood of teach->codes, whose vectors it replaces.  qerror: NULL, or [epochs] for the quantization error
 * (find_qerror's sum) of the map every epoch started from.  0, or 1 after a message.
 * buffer > 0: per epoch the data goes through the engine `buffer` rows at a time (somhip_batchmap_begin / _accumulate /
 * _finish), each piece a data set of its own -- uploaded, or generated in place for a gen: source -- that is destroyed
 * once it is taken: the device never holds more than `buffer` rows, and the result is the same, bit for bit. */
int som_batchmap_training(struct teach_params *teach, long epochs, long buffer, float *qerror);
/* bsom -missing: the same over data whose samples may leave components out (somhip_som_batchmap_missing; with buffer > 0
 * somhip_batchmap_missing_begin / _accumulate / _finish): a component of a model vector becomes the weighted mean of the
 * samples that know it.  On data without masks the result is som_batchmap_training's, bit for bit. */
int som_batchmap_missing_training(struct teach_params *teach, long epochs, long buffer, float *qerror);
/* bsom -gpus G: the data's rows in G blocks, one per rank, every rank the whole map (somhip_som_batchmap_ranks); rank 0
 * ends with the map in teach->codes and the epochs' qerror in qerror ([epochs]) and runs after(teach, arg) -- print, save */
int som_batchmap_training_multi(struct teach_params *teach, long epochs, float *qerror, int gpus,
                                int (*after)(struct teach_params *, void *), void *arg);
/* batch GLVQ (somhip_glvq_train): `epochs` epochs over all of teach->data at rates from teach->alpha down, sigmoid_beta 0
 * for the identity, on the labelled rows of teach->codes, which it replaces.  cost, correct: NULL, or [epochs] for the cost
 * and the number of correctly classified rows of the codebook every epoch started from.  0, or 1 after a message. */
int glvq_training(struct teach_params *teach, long epochs, float sigmoid_beta, double *cost, int64_t *correct);
/* the same run with the data going through the engine `buffer` rows at a time, every epoch (somhip_glvq_begin / _accumulate
 * / _finish): each piece a data set of its own with its labels, uploaded and destroyed once it is taken, so the device
 * never holds more than `buffer` data rows; the codebook, cost and correct are the plain run's, bit for bit */
int glvq_training_buffered(struct teach_params *teach, long epochs, long buffer, float sigmoid_beta, double *cost, int64_t *correct);
/* glvq -gpus G: the data's rows in G contiguous blocks, one per rank, every rank the whole codebook
 * (somhip_glvq_train_ranks); rank 0 ends with the codebook in teach->codes and the epochs' cost and correct ([epochs] or
 * NULL) and runs after(teach, arg) -- print, save */
int glvq_training_multi(struct teach_params *teach, long epochs, float sigmoid_beta, double *cost, int64_t *correct, int gpus,
                        int (*after)(struct teach_params *, void *), void *arg);
/* batch GRLVQ (somhip_grlvq_train): glvq_training under the relevance-weighted metric.  lambda ([dim], in and out): the
 * relevances, taken as they are and left as the run ends; eps: their rate.  epochs 0: nothing is trained.  Then one more
 * search (somhip_grlvq_search): *final_cost and *final_correct describe teach->codes under lambda as the call leaves them. */
int grlvq_training(struct teach_params *teach, long epochs, float sigmoid_beta, float eps, float *lambda, double *cost, int64_t *correct,
                   double *final_cost, int64_t *final_correct);
/* batch GMLVQ (somhip_gmlvq_train): glvq_training under d(x, w) = |Omega (x - w)|^2.  omega ([rank][dim], in and out): the
 * matrix, taken as it is and left as the run ends; eps: its rate.  epochs 0: nothing is trained.  Then one more search
 * (somhip_gmlvq_search): *final_cost and *final_correct describe teach->codes under omega as the call leaves them.
 * projected: NULL, or [rows of the data][rank] for the data under that omega (somhip_gmlvq_project). */
int gmlvq_training(struct teach_params *teach, long epochs, float sigmoid_beta, float eps, float *omega, int rank, double *cost,
                   int64_t *correct, double *final_cost, int64_t *final_correct, float *projected);
/* batch Robust Soft LVQ (somhip_rslvq_train): `epochs` epochs over all of teach->data at rates from teach->alpha down, under
 * a mixture of squared width sigma2, on the labelled rows of teach->codes, which it replaces.  epochs 0: nothing is trained.
 * cost, correct: NULL, or [epochs] for the figures of the codebook every epoch started from.  Then one evaluation
 * (somhip_rslvq_search): *final_cost and *final_correct describe teach->codes as the call leaves them; pown: NULL, or
 * [rows of the data] for P(label | x) under them.  0, or 1 after a message. */
int rslvq_training(struct teach_params *teach, long epochs, float sigma2, double *cost, int64_t *correct, double *final_cost,
                   int64_t *final_correct, double *pown);
/* batch neural gas (somhip_ng_train): `epochs` epochs over all of teach->data, lambda from lambda0 down to lambda_end,
 * ranks 0 for the engine's rule, on the rows of teach->codes, which it replaces (lattice and labels play no part).  line:
 * NULL, or [epochs] for each epoch's lambda and ranks as the engine forms them and the quantization error (find_qerror's sum)
 * of the codebook the epoch started from.  0, or 1 after a message. */
struct ng_line { double lambda; int ranks; float qerror; };
int ng_training(struct teach_params *teach, long epochs, double lambda0, double lambda_end, long ranks, struct ng_line *line);
/* ... over every rank (somhip_ng_train_dense): the same run with no truncation, on a codebook of at most SOMHIP_NG_DENSE_MAX
 * rows; a line's ranks is the number of rows */
int ng_training_dense(struct teach_params *teach, long epochs, double lambda0, double lambda_end, struct ng_line *line);
/* winners of every data row (the scan behind compute_accuracy / find_labels) */
int find_all_winners(struct teach_params *teach, int32_t *index, float *diff, int32_t *ret);
/* the k nearest codes of every data row (knntest): k <= 8 */
int find_all_knn(struct entries *codes, struct entries *data, int knn, int32_t *index, float *diff);
/* the class vote over them, formed on the engine (setlabel, elimin; eveninit/propinit and balance through
 * knn_correct_all): k <= SOMHIP_KNN_MAX */
int knn_vote_all(struct entries *codes, struct entries *data, int knn, int32_t *label, int32_t *freq, int32_t *own,
                 int32_t *found);
unsigned char *knn_correct_all(struct entries *data, int knn);
struct entries *pick_rows(struct entries *src, const long *rows, long n);
struct entries *lininit_codes(struct entries *data, int topol, int neigh, int xdim, int ydim);
struct entries *randinit_codes(struct entries *data, int topol, int neigh, int xdim, int ydim);
/* ---- within-class distance statistics (balance, mindist, stddev; lvq_rout.c:384-491, 918-1004) ---- */
struct mindists { long num_classes; long *cls; long *noe; float *dists; float *devs; };   /* devs: NULL until deviations() */
struct mindists *med_distances(struct entries *codes);          /* the nearest-neighbour search runs on the engine */
int deviations(struct entries *data, struct mindists *md);      /* 0, or 1 after naming a label of data md has no class for */
void free_mindists(struct mindists *md);
/* ---- what every tool does before the engine is involved ---- */
struct pak_inputs { struct entries *data, *codes; };
/* opens -din then -cin with the reference's messages; fmt strings take the file name.  need_map:
 * the codebook must be a hexa/rect map.  Returns 0 or 1 (after closing what it opened). */
int pak_open_inputs(const char *din, int data_labels, const char *data_fail_fmt, const char *cin, int code_labels,
                    const char *code_fail_fmt, int need_map, struct pak_inputs *io);
/* options shared by the training tools: -din -cin -cout -rlen -rand -buffer -alpha_type -selfuncs
 * -snapfile -snapinterval (vsom.c:77-131, lvqtrain.c:115-142) */
struct pak_train_cli {
  char *din, *cin, *cout, *rand_s, *alpha_s, *funcname;
  long length, buffer;
  struct snapshot_info snap;
  int want_snapshots;
};
void pak_train_cli(int argc, char **argv, struct pak_train_cli *o);
/* init_random(-rand) and the data order it asks for: one shuffle of the whole file, or per-buffer
 * reshuffling when -buffer is smaller than the file (datafile.c:237-344) */
void pak_apply_rand(struct entries *data, const char *rand_s, long buffer);
/* ---- the batch tools' shared front end (bsom, bng, glvq, grlvq, gmlvq, rslvq; pak_io.c): the options, refusals and
 * report lines they have in common, each stated once under the tool's name `tool` ---- */
/* -v as the batch tools read it: 1 when -v is given (per-epoch lines are wanted); global_options sets the level, and a
 * bare -v, whose next argument is no level, leaves it at 1 */
int pak_batch_verbose(int argc, char **argv);
/* exits with "tool: option value is negative or not a number" unless value >= 0 */
void pak_rate_check(const char *tool, const char *option, float value);
/* 1 after a message when the codebook, then the data, has masked components; data_tail: what the data's message ends
 * in after "not supported", or NULL where masked data are taken (bsom -missing) */
int pak_masked_inputs(const char *tool, const struct pak_inputs *io, const char *cin, const char *din, const char *data_tail);
/* 1 after a message, in this order, for: a codebook row without a label, a data row without one, a codebook whose rows
 * carry one label, a data row whose label no codebook row carries */
int pak_labelled_inputs(const char *tool, const struct pak_inputs *io, const char *cin, const char *din);
/* -buffer N and -gpus G of bsom and glvq: extracted, then refused with an exit when -buffer is given below
 * least_buffer or -gpus lies outside 1 .. 64 (what the pair means together is the tool's to say) */
struct pak_pieces_cli { char *buffer_s, *gpus_s; long buffer; int gpus; };
void pak_pieces_cli(int argc, char **argv, const char *tool, long least_buffer, struct pak_pieces_cli *o);
/* the engines' rate of epoch t of `epochs`, from a down to 0, and their radius, from r down to 1: these expressions, in
 * this association, are what the engines compute */
float pak_linear_rate(float a, long epochs, long t);
float pak_linear_radius(float r, long epochs, long t);
/* the per-epoch lines of the GLVQ family (eps: NULL, or the second rate for its column; nothing where cost is NULL) and
 * the line of the final figures, over `rows` data rows */
void pak_print_epoch_costs(FILE *fp, long epochs, float alpha, const float *eps, const double *cost, const int64_t *correct, long rows);
void pak_print_final_cost(FILE *fp, double cost, int64_t correct, long rows);
/* says at -v 2 where the codebook goes, and saves it: 0, or 1 */
int pak_save_codes(struct entries *codes, const char *cout);
void pak_shutdown(void);
/* vsom -gpus G: one process per GPU, codebook sharded, RCCL all-reduce of the winner keys (pak_ranks.c).  Must be called
 * before this process has used a GPU; rank 0 runs after(teach, arg) (save the codebook) when training succeeded. */
int som_training_multi(struct teach_params *teach, int gpus, int (*after)(struct teach_params *, void *), void *arg);
/* lvqtrain -gpus G: rows of the codebook sharded over the ranks, exact (pak_ranks.c) */
int lvq_training_multi(struct teach_params *teach, int kind, float winlen, float epsilon, float clamp, float *talpha, int gpus,
                       int (*after)(struct teach_params *, void *), void *arg);
/* the launcher behind it, for tools that spread independent work over the GPUs (vfind -gpus G: trials as replicas) */
int pak_run_ranks(int world, int (*rank_main)(int rank, int world, int *fds, void *arg), void *arg);
int pak_rank_device(int rank);          /* selects GPU rank % (visible GPUs) for this process's engine; -1 on failure */
int pak_sock_write(int fd, const void *b, size_t n);
int pak_sock_read(int fd, void *b, size_t n);

#endif
