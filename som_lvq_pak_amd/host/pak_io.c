/* pak_io.c -- the part of the tools' host library that needs no GPU: arguments, labels, hit lists, the .dat/.cod
 * text files with the "#!somf32" side format and the gen: generator, the .lra rate files, the reference's LCG and
 * -rand shuffle, the alpha schedules, the tools' shared front end and the batch tools' own.  Links with -lm alone
 * (pak_engine.c and pak_ranks.c hand the hot path to libsomhip.so).  Written from scratch over dense storage; file
 * formats, flag names, messages and numerics follow SOM_PAK/LVQ_PAK 3.2 (citations: file:line in hynde/som_lvq_pak). */
#define _GNU_SOURCE
#include "pak_int.h"

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>
#include <unistd.h>

/* ------------------------------------------------------------------ arguments */
int verbose_level = 1;
int use_fixed_level = 0, use_weights_level = 0;

/* lvq_pak.c:583-612: linear search, the value is the next argv; OPTION2 flags take none */
char *extract_parameter(int argc, char **argv, const char *param, int when)
{
  int i = 0;
  while (i < argc && strcmp(param, argv[i]) != 0) i++;
  if (i <= argc - 1 && when == OPTION2) return "";
  if (i < argc - 1) return argv[i + 1];
  if (when == ALWAYS) {
    fprintf(stderr, "Can't find asked option %s\n", param);
    exit(-1);
  }
  return NULL;
}
long oatoi(const char *s, long def) { return s ? atol(s) : def; }
float oatof(const char *s, float def) { return s ? (float)atof(s) : def; }

static const char *masked_string = "x";          /* datafile.h:33, -mask_str / LVQSOM_MASK_STR */

int global_options(int argc, char **argv)        /* lvq_pak.c:618-660 */
{
  char *s = getenv("LVQSOM_MASK_STR");
  if (s) masked_string = s;
  s = extract_parameter(argc, argv, "-mask_str", OPTION);
  if (s) masked_string = s;
  if (extract_parameter(argc, argv, "-version", OPTION2))
    fprintf(stderr, "Version: som_lvq_pak_amd (MI355X engine, libsomhip %d), file formats of SOM/LVQ_PAK 3.2\n",
            SOMHIP_VERSION);      /* the header's number: tools and library are built from one tree */
  verbose_level = (int)oatoi(extract_parameter(argc, argv, "-v", OPTION), 1);
  return 0;
}

const char *pak_progname(const char *argv0)      /* fileio.c:433-465: basename of argv[0] */
{
  const char *p = strrchr(argv0, '/');
  return p ? p + 1 : argv0;
}

/* ------------------------------------------------------------------ labels */
static char **label_names = NULL;                /* [0] unused: 0 = LABEL_EMPTY */
static int label_count = 0, label_cap = 0;

int find_conv_to_ind(const char *str)
{
  for (int i = 1; i <= label_count; i++)
    if (strcmp(label_names[i], str) == 0) return i;
  if (label_count + 2 > label_cap) {
    label_cap = label_cap ? 2 * label_cap : 64;
    label_names = realloc(label_names, sizeof(char *) * label_cap);
  }
  label_names[++label_count] = strdup(str);
  return label_count;
}
const char *find_conv_to_lab(int ind) { return (ind >= 1 && ind <= label_count) ? label_names[ind] : NULL; }
int number_of_labels(void) { return label_count; }

struct hitlist *new_hitlist(void) { return calloc(1, sizeof(struct hitlist)); }
void free_hitlist(struct hitlist *h) { if (h) { free(h->label); free(h->freq); free(h); } }
long add_hit(struct hitlist *h, long label)
{
  long i;
  for (i = 0; i < h->entries; i++) if (h->label[i] == label) break;
  if (i == h->entries) {
    if (h->entries == h->cap) {
      h->cap = h->cap ? 2 * h->cap : 8;
      h->label = realloc(h->label, sizeof(long) * h->cap);
      h->freq = realloc(h->freq, sizeof(long) * h->cap);
    }
    h->label[i] = label; h->freq[i] = 1; h->entries++;
    return 1;
  }
  long f = ++h->freq[i];
  while (i > 0 && h->freq[i - 1] < f) {          /* strictly smaller: ties keep their order */
    long tl = h->label[i - 1], tf = h->freq[i - 1];
    h->label[i - 1] = h->label[i]; h->freq[i - 1] = h->freq[i];
    h->label[i] = tl; h->freq[i] = tf;
    i--;
  }
  return f;
}
long hitlist_label_freq(struct hitlist *h, long label)
{
  for (long i = 0; i < h->entries; i++) if (h->label[i] == label) return h->freq[i];
  return 0;
}

/* ------------------------------------------------------------------ files */
static const char *topol_names[] = {NULL, "data", "lvq", "hexa", "rect"};
static const char *neigh_names[] = {NULL, "bubble", "gaussian"};

static int id_of(const char **names, int n, const char *s)
{
  if (s) for (int i = 1; i < n; i++) if (strcasecmp(names[i], s) == 0) return i;
  return 0;
}

static FILE *open_text(const char *name, const char *mode, int *is_pipe)
{
  size_t len = strlen(name);
  *is_pipe = 0;
  if (strcmp(name, "-") == 0) return mode[0] == 'r' ? stdin : stdout;
  int gz = (len > 3 && strcmp(name + len - 3, ".gz") == 0) ||
           (len > 2 && (strcmp(name + len - 2, ".z") == 0 || strcmp(name + len - 2, ".Z") == 0));
  if (gz) {                                      /* fileio.c:57-200: compressed files through gzip */
    char cmd[4096];
    snprintf(cmd, sizeof cmd, mode[0] == 'r' ? "gzip -d -c %s" : "gzip -9 -c >%s", name);
    *is_pipe = 1;
    return popen(cmd, mode[0] == 'r' ? "r" : "w");
  }
  return fopen(name, mode);
}
static void close_text(FILE *fp, int is_pipe)
{
  if (fp == stdin || fp == stdout) return;
  if (is_pipe) pclose(fp); else fclose(fp);
}

void clear_entry_labels(struct entries *e, long r)
{
  free(e->rows[r].labels);
  e->rows[r].labels = NULL;
  e->rows[r].num_labs = 0;
}
void add_entry_label(struct entries *e, long r, int label)
{
  struct data_entry *d = &e->rows[r];
  d->labels = realloc(d->labels, sizeof(int) * (d->num_labs + 1));
  d->labels[d->num_labs++] = label;
}

/* One vector component, with the value sscanf("%f") gives (the reference's load_entry,
 * datafile.c:627, 664): correctly rounded to float.  Plain decimals -- at most 19 significant
 * digits, mantissa below 2^53, |power of ten| <= 22 -- are formed with ONE double operation
 * (m * 10^e or m / 10^e, both operands exact, so the double is the correctly rounded value) and
 * then narrowed; the only way the second rounding can go wrong is a double that sits exactly on a
 * float tie, and that case, like everything unusual (hex, inf/nan, long digit strings, trailing
 * characters, float under/overflow), goes to sscanf itself.  ~10x faster than sscanf per token. */
int pak_parse_float(const char *s, float *out)
{
  static const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14,
                                 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  const char *p = s;
  int neg = 0, nd = 0, any = 0, e10 = 0;
  unsigned long long m = 0;
  if (*p == '-') { neg = 1; p++; } else if (*p == '+') p++;
  for (; *p >= '0' && *p <= '9'; p++) {
    any = 1;
    if (nd == 0 && *p == '0') continue;
    if (nd >= 19) goto slow;
    m = m * 10 + (unsigned)(*p - '0'); nd++;
  }
  if (*p == '.') {
    p++;
    for (; *p >= '0' && *p <= '9'; p++) {
      any = 1;
      e10--;
      if (nd == 0 && *p == '0') continue;
      if (nd >= 19) goto slow;
      m = m * 10 + (unsigned)(*p - '0'); nd++;
    }
  }
  if (!any) goto slow;
  if (*p == 'e' || *p == 'E') {
    p++;
    int eneg = 0, ex = 0, ed = 0;
    if (*p == '-') { eneg = 1; p++; } else if (*p == '+') p++;
    for (; *p >= '0' && *p <= '9'; p++) { if (ex < 10000) ex = ex * 10 + (*p - '0'); ed++; }
    if (!ed) goto slow;
    e10 += eneg ? -ex : ex;
  }
  if (*p != '\0') goto slow;
  if (m == 0) { *out = neg ? -0.0f : 0.0f; return 1; }
  if (m >= (1ULL << 53) || e10 < -22 || e10 > 22) goto slow;
  {
    double d = (double)m;
    d = e10 >= 0 ? d * p10[e10] : d / p10[-e10];
    if (!(d >= 1.2e-38 && d <= 3.4e38)) goto slow;          /* keep clear of the float range limits */
    unsigned long long bits;
    memcpy(&bits, &d, sizeof bits);
    if ((bits & 0x1FFFFFFFULL) == 0x10000000ULL) goto slow;  /* exactly on a float tie: let strtof decide */
    *out = (float)(neg ? -d : d);
    return 1;
  }
slow:
  return sscanf(s, "%f", out) > 0;
}

/* what may follow the numbers of a row: labels, weight=N, fixed=X,Y (datafile.c:705-735) */
static int row_tokens(struct entries *e, long r, char *tok, char **save, struct fixpoint *fix, int *any_weight,
                      int *any_fixed, int labels_needed, long lineno, const char *name)
{
  struct data_entry *d = &e->rows[r];
  int label_found = 0;
  for (; tok; tok = strtok_r(NULL, " \r\t", save)) {
    if (strncmp(tok, "weight=", 7) == 0) { d->weight = (short)atoi(tok + 7); *any_weight = 1; }
    else if (strncmp(tok, "fixed=", 6) == 0) {
      char *comma = strchr(tok, ',');
      if (!comma) { fprintf(stderr, "bad fixed point, line %ld of file %s\n", lineno, name); return 1; }
      fix->xfix = (short)atoi(tok + 6);
      fix->yfix = (short)atoi(comma + 1);
      *any_fixed = 1;
    } else {
      add_entry_label(e, r, find_conv_to_ind(tok));
      label_found++;
    }
  }
  if (labels_needed && !label_found) {
    fprintf(stderr, "Required label missing on line %ld of file %s\n", lineno, name);
    return 1;
  }
  return 0;
}

static int parse_header(struct entries *e, const char *line, const char *name)
{
  int dim = 0;
  if (sscanf(line, "%d", &dim) <= 0 || dim <= 0) {
    fprintf(stderr, "Can't read dimension parameter in file %s", name);
    return 0;
  }
  char *save, *dup = strdup(line);
  strtok_r(dup, " ", &save);
  char *t = strtok_r(NULL, " ", &save);
  char *xs = strtok_r(NULL, " ", &save), *ys = strtok_r(NULL, " ", &save), *ns = strtok_r(NULL, " ", &save);
  e->dimension = (short)dim;
  e->topol = (short)id_of(topol_names, 5, t);
  e->xdim = xs ? (short)atoi(xs) : 0;
  e->ydim = ys ? (short)atoi(ys) : 0;
  e->neigh = (short)id_of(neigh_names, 3, ns);
  free(dup);
  return dim;
}

/* dense side arrays + row views once all rows are in e->points (maskrows / fixtmp may be NULL) */
static void finish_entries(struct entries *e, char **maskrows, struct fixpoint *fixtmp, int any_fixed, int any_weight)
{
  long n = e->num_entries;
  int dim = e->dimension, any_mask = 0;
  for (long r = 0; maskrows && r < n; r++) any_mask |= maskrows[r] != NULL;
  if (any_mask) e->masks = calloc((size_t)n * dim + 1, 1);
  if (any_fixed) e->fixed_xy = malloc(sizeof(short) * 2 * (n + 1));
  if (any_weight) e->weights = malloc(sizeof(short) * (n + 1));
  for (long r = 0; r < n; r++) {
    struct data_entry *d = &e->rows[r];
    d->points = e->points + r * dim;
    if (any_mask && maskrows[r]) { memcpy(e->masks + r * dim, maskrows[r], dim); d->mask = e->masks + r * dim; }
    if (maskrows) free(maskrows[r]);
    if (any_fixed) {
      e->fixed_xy[2 * r] = fixtmp[r].xfix; e->fixed_xy[2 * r + 1] = fixtmp[r].yfix;
      if (fixtmp[r].xfix >= 0) d->fixed = (struct fixpoint *)(e->fixed_xy + 2 * r);
    }
    if (any_weight) e->weights[r] = d->weight;
  }
}

static void write_header(FILE *fp, const struct entries *c)   /* datafile.c:396-415 */
{
  fprintf(fp, "%d", c->dimension);
  if (c->topol > TOPOL_DATA) {
    fprintf(fp, " %s", topol_names[c->topol]);
    if (c->topol > TOPOL_LVQ) fprintf(fp, " %d %d %s", c->xdim, c->ydim, neigh_names[c->neigh] ? neigh_names[c->neigh] : "");
  }
  fputc('\n', fp);
}

/* ---- raw fp32 side format (the text parser is the wall once the kernels are fast) ----
 *   line 1   "#!somf32 <rows> <flags>"         flags bit 0: a text section follows the numbers
 *   line 2   the .dat header line              "<dim> [topol [xdim ydim neigh]]"  (datafile.c:396-415)
 *   payload  rows * dim little-endian float32  NaN = masked component (the 'x' of the text format)
 *   text     (flag bit 0) one line per row with what follows the numbers in a .dat row: labels, weight=, fixed=
 * Read with one fread straight into the dense array; rows whose components are all masked are dropped as in
 * the text reader.  `datconv` converts both ways. */
static struct entries *read_f32(FILE *fp, const char *first_line, const char *name, int labels_needed, int skip_empty)
{
  long n = 0;
  int flags = 0;
  if (sscanf(first_line, "#!somf32 %ld %d", &n, &flags) < 1 || n < 0) { fprintf(stderr, "bad somf32 header in file %s\n", name); return NULL; }
  struct entries *e = calloc(1, sizeof *e);
  e->labels_needed = labels_needed;
  char *line = NULL;
  size_t cap = 0;
  struct fixpoint *fixtmp = NULL;
  char **maskrows = NULL;
  int any_fixed = 0, any_weight = 0, dim;
  if (getline(&line, &cap, fp) < 0) goto fail;
  { size_t L = strlen(line); while (L && (line[L - 1] == '\n' || line[L - 1] == '\r')) line[--L] = 0; }
  if (!(dim = parse_header(e, line, name))) goto fail;
  e->points = malloc(sizeof(float) * (size_t)(n ? n : 1) * dim);
  e->rows = calloc((size_t)(n ? n : 1), sizeof(struct data_entry));
  if (fread(e->points, sizeof(float) * dim, (size_t)n, fp) != (size_t)n) { fprintf(stderr, "file %s is shorter than its header says\n", name); goto fail; }
  maskrows = calloc((size_t)(n ? n : 1), sizeof(char *));
  fixtmp = malloc(sizeof(struct fixpoint) * (size_t)(n ? n : 1));
  long kept = 0;
  for (long r = 0; r < n; r++) {                    /* NaN -> mask; drop empty rows; compact in place */
    float *p = e->points + r * dim;
    char *mask = NULL;
    int maskcnt = 0;
    for (int i = 0; i < dim; i++)
      if (p[i] != p[i]) { if (!mask) mask = calloc(dim, 1); mask[i] = 1; maskcnt++; p[i] = 0.0f; }
    char *tokline = NULL, *save = NULL, *tok = NULL;
    if (flags & 1) {
      if (getline(&line, &cap, fp) < 0) { fprintf(stderr, "file %s: text section ends at row %ld\n", name, r); free(mask); goto fail; }
      size_t L = strlen(line);
      if (L && line[L - 1] == '\n') line[--L] = 0;
      tokline = line;
    }
    if (maskcnt == dim && skip_empty) { free(mask); continue; }
    if (kept != r) memmove(e->points + kept * dim, p, sizeof(float) * dim);
    maskrows[kept] = mask;
    fixtmp[kept].xfix = fixtmp[kept].yfix = -1;
    e->num_entries = kept + 1;
    if (tokline) tok = strtok_r(tokline, " \r\t", &save);
    if (row_tokens(e, kept, tok, &save, &fixtmp[kept], &any_weight, &any_fixed, labels_needed, r + 3, name)) goto fail;
    kept++;
  }
  e->num_entries = kept;
  finish_entries(e, maskrows, fixtmp, any_fixed, any_weight);
  free(maskrows); free(fixtmp); free(line);
  return e;
fail:
  free(maskrows); free(fixtmp); free(line);
  close_entries(e);
  return NULL;
}

int save_entries_f32(struct entries *c, const char *name)
{
  int is_pipe, any_text = 0;
  for (long r = 0; r < c->num_entries && !any_text; r++)
    any_text = c->rows[r].num_labs > 0 || c->rows[r].weight != 0 || c->rows[r].fixed != NULL;
  FILE *fp = open_text(name, "w", &is_pipe);
  if (!fp) { fprintf(stderr, "Can't open file %s for writing\n", name); return 1; }
  fprintf(fp, "#!somf32 %ld %d\n", c->num_entries, any_text);
  write_header(fp, c);
  const int dim = c->dimension;
  float *tmp = malloc(sizeof(float) * dim);
  for (long r = 0; r < c->num_entries; r++) {
    const struct data_entry *d = &c->rows[r];
    if (d->mask) {
      for (int i = 0; i < dim; i++) tmp[i] = d->mask[i] ? __builtin_nanf("") : d->points[i];
      fwrite(tmp, sizeof(float), dim, fp);
    } else fwrite(d->points, sizeof(float), dim, fp);
  }
  free(tmp);
  for (long r = 0; any_text && r < c->num_entries; r++) {
    const struct data_entry *d = &c->rows[r];
    for (int k = 0; k < d->num_labs; k++) fprintf(fp, "%s ", find_conv_to_lab(d->labels[k]));
    if (d->weight) fprintf(fp, "weight=%d ", d->weight);
    if (d->fixed) fprintf(fp, "fixed=%d,%d ", d->fixed->xfix, d->fixed->yfix);
    fputc('\n', fp);
  }
  int bad = ferror(fp);
  close_text(fp, is_pipe);
  return bad;
}

/* ---- seeded generator as a data source:  -din gen:k=256,dim=512,n=100000,seed=3456[,labels=1] ----
 * The Gaussian-mixture stream of SURVEY 8(d), counter-based so that any row can be produced anywhere (host here,
 * k_gen_mixture on the device: same bits, tests/test_gpu_parity.py):  splitmix64(seed ^ counter) words; a centre
 * component is 4 z, a sample is centre[k(row)] + z with k(row) = word(seed_assign ^ row) mod K; z is the classic
 * sum of twelve uniforms minus six, here twelve 16-bit fields of three words: integer arithmetic and one exact
 * division by 65536, so host and device cannot differ (a Box-Muller z would depend on each side's log and cos).
 * labels=1 attaches the mixture id ("c<k>") as the row's label. */
uint64_t pak_splitmix64(uint64_t x)
{
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}
float pak_gen_z(uint64_t seed, uint64_t counter)
{
  int32_t sum = 0;
  for (int w = 0; w < 3; w++) {
    uint64_t v = pak_splitmix64(seed ^ (3 * counter + w));
    sum += (int32_t)(v & 0xFFFF) + (int32_t)((v >> 16) & 0xFFFF) + (int32_t)((v >> 32) & 0xFFFF) + (int32_t)(v >> 48);
  }
  return (float)(sum - 6 * 65535) / 65536.0f;      /* |sum - 393210| < 2^24: exact */
}
static int gen_centre(uint64_t seed, int k_centres, long row)
{
  return (int)(pak_splitmix64(seed ^ 0xB492B66FBE98F273ULL ^ (uint64_t)row) % (uint64_t)k_centres);
}
void pak_gen_row(uint64_t seed, int k_centres, int dim, long row, float *out, int *centre)
{
  const uint64_t seed_c = seed ^ 0xC3A5C85C97CB3127ULL;
  const int k = gen_centre(seed, k_centres, row);
  for (int i = 0; i < dim; i++) {
    const float mu = 4.0f * pak_gen_z(seed_c, (uint64_t)k * dim + i);
    out[i] = mu + pak_gen_z(seed, (uint64_t)row * dim + i);
  }
  if (centre) *centre = k;
}
int pak_parse_gen(const char *spec, long *n, int *dim, int *k, uint64_t *seed, int *labels)
{
  if (strncmp(spec, "gen:", 4) != 0) return 0;
  *n = 0; *dim = 0; *k = 16; *seed = 1234; *labels = 0;
  char *dup = strdup(spec + 4), *save, *tok;
  for (tok = strtok_r(dup, ",", &save); tok; tok = strtok_r(NULL, ",", &save)) {
    if (sscanf(tok, "n=%ld", n) == 1 || sscanf(tok, "dim=%d", dim) == 1 || sscanf(tok, "k=%d", k) == 1 ||
        sscanf(tok, "labels=%d", labels) == 1) continue;
    unsigned long long sv;
    if (sscanf(tok, "seed=%llu", &sv) == 1) { *seed = sv; continue; }
    fprintf(stderr, "gen: unknown field '%s' (n=, dim=, k=, seed=, labels=)\n", tok);
    free(dup);
    return -1;
  }
  free(dup);
  if (*n <= 0 || *dim <= 0 || *dim > 32767 || *k <= 0) { fprintf(stderr, "gen: needs n=, dim= (and k > 0)\n"); return -1; }
  return 1;
}
int pak_gen_unlabelled(const char *name)
{
  long n; int dim, k, labels; uint64_t seed;
  return strncmp(name, "gen:", 4) == 0 && pak_parse_gen(name, &n, &dim, &k, &seed, &labels) > 0 && !labels;
}
int pak_gen_virtual_ok = 0;

/* host rows of a virtual source (same stream, same bits as the device's); counter-based: every row is independent, so
 * the rows are made in parallel */
int pak_materialize(struct entries *e)
{
  if (!e || !e->is_virtual) return 0;
  const long n = e->num_entries;
  const int dim = e->dimension;
  e->points = malloc(sizeof(float) * (size_t)n * dim);
  e->rows = calloc((size_t)n, sizeof(struct data_entry));
  if (!e->points || !e->rows) { fprintf(stderr, "gen: out of memory for %ld x %d host rows\n", n, dim); return 1; }
#pragma omp parallel for schedule(static)
  for (long r = 0; r < n; r++) pak_gen_row(e->gen_seed, e->gen_k, dim, r, e->points + r * dim, NULL);
  e->is_virtual = 0;
  finish_entries(e, NULL, NULL, 0, 0);
  return 0;
}

static struct entries *gen_entries(const char *spec)
{
  long n; int dim, k, labels; uint64_t seed;
  if (pak_parse_gen(spec, &n, &dim, &k, &seed, &labels) <= 0) return NULL;
  struct entries *e = calloc(1, sizeof *e);
  e->dimension = (short)dim;
  e->num_entries = n;
  e->is_virtual = 1; e->gen_seed = seed; e->gen_k = k;
  if (pak_gen_virtual_ok && !labels) return e;         /* kept as a specification: the engine generates it in HBM */
  if (pak_materialize(e)) { close_entries(e); return NULL; }
  /* the label table is not thread-safe: labels are attached after the parallel rows, in row order, which is also the
   * order the text reader would meet them in */
  for (long r = 0; labels && r < n; r++) {
    char nm[32];
    snprintf(nm, sizeof nm, "c%d", gen_centre(seed, k, r));
    add_entry_label(e, r, find_conv_to_ind(nm));
  }
  return e;
}

/* open_entries + read_entries (datafile.c:191,237) for a whole file.  Header: first
 * non-comment line "<dim> [topol [xdim ydim neigh]]" (datafile.c:112-145).  Rows: <dim>
 * numbers or the mask string, then labels / weight=N / fixed=X,Y (datafile.c:552-748);
 * '#' lines and blank lines are skipped; rows with every component masked are dropped
 * when skip_empty (datafile.c:677-686). */
struct entries *open_entries(const char *name, int labels_needed, int skip_empty)
{
  int is_pipe;
  if (strncmp(name, "gen:", 4) == 0) return gen_entries(name);
  FILE *fp = open_text(name, "r", &is_pipe);
  if (!fp) { fprintf(stderr, "Can't open file %s", name); return NULL; }
  struct entries *e = calloc(1, sizeof *e);
  e->labels_needed = labels_needed;
  char *line = NULL;
  size_t cap = 0;
  long lineno = 0, nalloc = 0;
  int have_header = 0, dim = 0;
  struct fixpoint *fixtmp = NULL;
  int any_fixed = 0, any_weight = 0;
  char **maskrows = NULL;

  while (getline(&line, &cap, fp) >= 0) {
    lineno++;
    size_t L = strlen(line);
    if (L && line[L - 1] == '\n') line[--L] = 0;
    if (lineno == 1 && strncmp(line, "#!somf32", 8) == 0) {      /* the raw fp32 side format */
      struct entries *b = read_f32(fp, line, name, labels_needed, skip_empty);
      free(line); free(e);
      close_text(fp, is_pipe);
      return b;
    }
    if (line[0] == '#') continue;
    if (!have_header) {
      if (!(dim = parse_header(e, line, name))) goto fail;
      have_header = 1;
      continue;
    }
    char *save;
    char *tok = strtok_r(line, " \r\t", &save);
    if (!tok) continue;                          /* empty line */
    if (e->num_entries == nalloc) {
      nalloc = nalloc ? 2 * nalloc : 1024;
      e->points = realloc(e->points, sizeof(float) * nalloc * dim);
      e->rows = realloc(e->rows, sizeof(struct data_entry) * nalloc);
      maskrows = realloc(maskrows, sizeof(char *) * nalloc);
      fixtmp = realloc(fixtmp, sizeof(struct fixpoint) * nalloc);
    }
    long r = e->num_entries;
    float *p = e->points + r * dim;
    char *mask = NULL;
    int maskcnt = 0;
    for (int i = 0; i < dim; i++) {
      if (i > 0) tok = strtok_r(NULL, " \r\t", &save);
      if (!tok) {
        fprintf(stderr, "load_entry: can't read entry in file %s on line %ld, component %d\n", name, lineno, i);
        goto fail;
      }
      if (strcmp(tok, masked_string) == 0) {
        if (!mask) mask = calloc(dim, 1);
        mask[i] = 1; maskcnt++; p[i] = 0.0f;
      } else if (!pak_parse_float(tok, &p[i])) {
        fprintf(stderr, "load_entry: can't read entry in file %s on line %ld, component %d\n", name, lineno, i);
        goto fail;
      }
    }
    if (maskcnt == dim && skip_empty) { free(mask); continue; }
    struct data_entry *d = &e->rows[r];
    memset(d, 0, sizeof *d);
    maskrows[r] = mask;
    fixtmp[r].xfix = fixtmp[r].yfix = -1;
    e->num_entries++;
    tok = strtok_r(NULL, " \r\t", &save);
    if (row_tokens(e, r, tok, &save, &fixtmp[r], &any_weight, &any_fixed, labels_needed, lineno, name)) goto fail;
  }
  if (!have_header) { fprintf(stderr, "Can't read file %s", name); goto fail; }
  finish_entries(e, maskrows, fixtmp, any_fixed, any_weight);
  free(maskrows); free(fixtmp); free(line);
  close_text(fp, is_pipe);
  return e;
fail:
  free(line);
  close_text(fp, is_pipe);
  return NULL;
}

static void free_rows(struct entries *e)
{
  for (long r = 0; e->rows && r < e->num_entries; r++) free(e->rows[r].labels);   /* (a virtual gen: source has no rows) */
  free(e->rows); free(e->points); free(e->masks); free(e->fixed_xy); free(e->weights);
}
void close_entries(struct entries *e)
{
  if (!e) return;
  if (e->drop_mirror) e->drop_mirror(e);               /* the per-sample surface's mirror (an orphan if the engine went first) */
  free_rows(e);
  free(e);
}

/* write_entry datafile.c:420-447: "%g " per value, "%s " per label */
static void write_rows(FILE *fp, struct entries *c, const char *comments)
{
  write_header(fp, c);
  if (comments) fputs(comments, fp);
  for (long r = 0; r < c->num_entries; r++) {
    struct data_entry *d = &c->rows[r];
    for (int i = 0; i < c->dimension; i++)
      if (d->mask && d->mask[i]) fprintf(fp, "%s ", masked_string);
      else fprintf(fp, "%g ", d->points[i]);
    for (int k = 0; k < d->num_labs; k++) {
      if (d->labels[k] == LABEL_EMPTY) break;
      fprintf(fp, "%s ", find_conv_to_lab(d->labels[k]));
    }
    fprintf(fp, "\n");
  }
}
int save_entries_wcomments(struct entries *codes, const char *name, const char *comments)
{
  int is_pipe;
  size_t nl = strlen(name);
  if (nl > 4 && strcmp(name + nl - 4, ".f32") == 0)      /* a name ending in .f32 asks for the raw fp32 side format */
    return save_entries_f32(codes, name);                /* (a 256x256x512 codebook is 400 MB of "%g" text otherwise)  */
  FILE *fp = open_text(name, "w", &is_pipe);
  if (!fp) { fprintf(stderr, "save_entries: Can't open file '%s'\n", name); return 1; }
  write_rows(fp, codes, comments);
  close_text(fp, is_pipe);
  return 0;
}

/* OLVQ1 learning-rate files, datafile.c:1030-1110: "<name up to the first '.'>.lra", one
 * "%g" per line */
static void lra_name(char *out, size_t n, const char *file)
{
  snprintf(out, n - 4, "%s", file);
  char *dot = strchr(out, '.');
  if (dot) *dot = 0;
  strcat(out, ".lra");
}
int alpha_read(float *alpha, long noc, const char *infile)
{
  char nm[2048];
  lra_name(nm, sizeof nm, infile);
  FILE *fp = fopen(nm, "r");
  if (!fp) { ifverbose(1) fprintf(stderr, "Can't open alpha file %s", nm); return 0; }
  for (long i = 0; i < noc; i++)
    if (fscanf(fp, "%g\n", &alpha[i]) < 0) { fclose(fp); return 0; }
  fclose(fp);
  return 1;
}
int alpha_write(float *alpha, long noc, const char *outfile)
{
  char nm[2048];
  lra_name(nm, sizeof nm, outfile);
  FILE *fp = fopen(nm, "w+");
  if (!fp) { fprintf(stderr, "Can't open alpha file %s for writing", nm); return 0; }
  for (long i = 0; i < noc; i++) fprintf(fp, "%g\n", alpha[i]);
  fclose(fp);
  return 0;
}
void invalidate_alphafile(const char *outfile)
{
  char nm[2048];
  lra_name(nm, sizeof nm, outfile);
  FILE *fp = fopen(nm, "r");
  if (fp) {
    ifverbose(1) fprintf(stdout, "Removing the learning rate file %s\n", nm);
    fclose(fp);
    if (remove(nm)) fprintf(stderr, "Can not remove %s", nm);
  }
}

/* a new entries block holding copies of the given rows of src (copy_entries + copy_entry,
 * datafile.c): header fields of src, vectors, masks and all labels */
struct entries *pick_rows(struct entries *src, const long *rows, long n)
{
  struct entries *e = calloc(1, sizeof *e);
  int dim = src->dimension;
  e->dimension = src->dimension; e->topol = src->topol; e->neigh = src->neigh;
  e->xdim = src->xdim; e->ydim = src->ydim; e->num_entries = n;
  e->points = malloc(sizeof(float) * (n > 0 ? n : 1) * dim);
  e->rows = calloc(n > 0 ? n : 1, sizeof(struct data_entry));
  if (src->masks) e->masks = calloc((n > 0 ? n : 1) * dim, 1);
  for (long k = 0; k < n; k++) {
    struct data_entry *s = &src->rows[rows[k]], *d = &e->rows[k];
    d->points = e->points + k * dim;
    memcpy(d->points, s->points, sizeof(float) * dim);
    if (e->masks && s->mask) { d->mask = e->masks + k * dim; memcpy(d->mask, s->mask, dim); }
    for (int l = 0; l < s->num_labs; l++) add_entry_label(e, k, s->labels[l]);
    d->weight = s->weight;
  }
  if (src->weights) {
    e->weights = malloc(sizeof(short) * (n + 1));
    for (long k = 0; k < n; k++) e->weights[k] = src->weights[rows[k]];
  }
  if (src->fixed_xy) {
    e->fixed_xy = malloc(sizeof(short) * 2 * (n + 1));
    for (long k = 0; k < n; k++) {
      e->fixed_xy[2 * k] = src->fixed_xy[2 * rows[k]]; e->fixed_xy[2 * k + 1] = src->fixed_xy[2 * rows[k] + 1];
      e->rows[k].fixed = e->fixed_xy[2 * k] >= 0 ? (struct fixpoint *)(e->fixed_xy + 2 * k) : NULL;
    }
  }
  return e;
}

/* ------------------------------------------------------------------ RNG, shuffle */
static unsigned long rnd_next = 1;
void init_random(int seed) { rnd_next = seed ? (unsigned long)seed : (unsigned long)(int)time(NULL); }
long orand(void) { rnd_next = (rnd_next * 23UL) % 100000001UL; return (long)(int)(rnd_next % 32767UL); }

/* rows first .. first+n-1 in shuffled order (datafile.c:1171-1177: for i in order, swap slot i with slot orand() % n) */
long *pak_shuffled_rows(long first, long n)
{
  long *perm = malloc(sizeof(long) * (n > 0 ? n : 1));
  for (long i = 0; i < n; i++) perm[i] = first + i;
  for (long i = 0; i < n; i++) { long j = orand() % n, t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
  return perm;
}

void randomize_entry_order(struct entries *e)          /* datafile.c:1152-1188 */
{
  if (e->num_entries <= 0) return;
  long *perm = pak_shuffled_rows(0, e->num_entries);
  struct entries *t = pick_rows(e, perm, e->num_entries);
  free_rows(e);
  e->points = t->points; e->rows = t->rows; e->masks = t->masks; e->fixed_xy = t->fixed_xy; e->weights = t->weights;
  free(t); free(perm);
}

/* ------------------------------------------------------------------ schedules (host scalars) */
float linear_alpha(long iter, long length, float alpha)      /* lvq_pak.c:903-906 */
{
  return alpha * (float)(length - iter) / (float)length;
}
float inverse_t_alpha(long iter, long length, float alpha)   /* lvq_pak.c:914-921 */
{
  float c = (float)length / 100.0f;
  return alpha * c / (c + (float)iter);
}
ALPHA_FUNC *alpha_func_by_name(const char *name, short *id)
{
  if (!name || strcasecmp(name, "linear") == 0) { *id = ALPHA_LINEAR; return linear_alpha; }
  if (strcasecmp(name, "inverse_t") == 0) { *id = ALPHA_INVERSE_T; return inverse_t_alpha; }
  *id = ALPHA_UNKNOWN;
  return NULL;
}

/* ------------------------------------------------------------------ shared tool front end */
int pak_open_inputs(const char *din, int data_labels, const char *data_fail_fmt, const char *cin, int code_labels,
                    const char *code_fail_fmt, int need_map, struct pak_inputs *io)
{
  io->data = io->codes = NULL;
  ifverbose(2) fprintf(stderr, "Input entries are read from file %s\n", din);
  if (!(io->data = open_entries(din, data_labels, 1))) { fprintf(stderr, data_fail_fmt, din); return 1; }
  ifverbose(2) fprintf(stderr, "Codebook entries are read from file %s\n", cin);
  if (!(io->codes = open_entries(cin, code_labels, 1))) { fprintf(stderr, code_fail_fmt, cin); goto bad; }
  if (need_map && io->codes->topol < TOPOL_HEXA) { fprintf(stderr, "File %s is not a map file\n", cin); goto bad; }
  if (io->data->dimension != io->codes->dimension) {
    fprintf(stderr, need_map == 2 ? "Data and codebook vectors have different dimensions (%d != %d)"
                                  : "Data and codebook vectors have different dimensions",
            io->data->dimension, io->codes->dimension);
    goto bad;
  }
  return 0;
bad:
  close_entries(io->data); close_entries(io->codes);
  io->data = io->codes = NULL;
  return 1;
}

void pak_train_cli(int argc, char **argv, struct pak_train_cli *o)
{
  memset(o, 0, sizeof *o);
  o->din = extract_parameter(argc, argv, "-din", ALWAYS);
  o->cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  o->cout = extract_parameter(argc, argv, "-cout", ALWAYS);
  o->length = oatoi(extract_parameter(argc, argv, "-rlen", ALWAYS), 1);
  o->rand_s = extract_parameter(argc, argv, "-rand", OPTION);
  o->buffer = oatoi(extract_parameter(argc, argv, "-buffer", OPTION), 0);
  o->alpha_s = extract_parameter(argc, argv, "-alpha_type", OPTION);
  o->funcname = extract_parameter(argc, argv, "-selfuncs", OPTION);
  o->snap.filename = extract_parameter(argc, argv, "-snapfile", OPTION);
  o->snap.interval = oatoi(extract_parameter(argc, argv, "-snapinterval", OPTION), 0);
  o->want_snapshots = o->snap.interval != 0;
  if (o->want_snapshots && !o->snap.filename) {
    o->snap.filename = o->cout;
    fprintf(stderr, "snapshot file not specified, using '%s'", o->snap.filename);
  }
}

void pak_apply_rand(struct entries *data, const char *rand_s, long buffer)
{
  init_random((int)oatoi(rand_s, 0));
  if (!rand_s) return;
  if (pak_materialize(data)) exit(1);                  /* a shuffle needs the rows on the host */
  if (buffer > 0 && buffer < data->num_entries) { data->buffer = buffer; data->random_order = 1; }   /* reshuffled per buffer */
  else randomize_entry_order(data);                                                               /* once, at load */
}

/* ------------------------------------------------------------------ the batch tools' shared front end */
int pak_batch_verbose(int argc, char **argv)
{
  int lines = extract_parameter(argc, argv, "-v", OPTION2) != NULL;
  global_options(argc, argv);
  char *level = extract_parameter(argc, argv, "-v", OPTION);
  if (lines && (!level || level[0] == '-')) verbose_level = 1;   /* a bare -v: the next argument is no level */
  return lines;
}

void pak_rate_check(const char *tool, const char *option, float value)
{
  if (!(value >= 0.0f)) { fprintf(stderr, "%s: %s %g is negative or not a number\n", tool, option, (double)value); exit(1); }
}

int pak_masked_inputs(const char *tool, const struct pak_inputs *io, const char *cin, const char *din, const char *data_tail)
{
  if (io->codes->masks) { fprintf(stderr, "%s: codebook %s has masked components (x): not supported\n", tool, cin); return 1; }
  if (io->data->masks && data_tail) { fprintf(stderr, "%s: data %s has masked components (x): not supported%s\n", tool, din, data_tail); return 1; }
  return 0;
}

/* 1 after a message when a row of e has no label */
static int unlabelled(const char *tool, const struct entries *e, const char *what, const char *name)
{
  for (long r = 0; r < e->num_entries; r++)
    if (get_entry_label(&e->rows[r]) == LABEL_EMPTY) {
      fprintf(stderr, "%s: %s %s has no labels on row %ld\n", tool, what, name, r);
      return 1;
    }
  return 0;
}

int pak_labelled_inputs(const char *tool, const struct pak_inputs *io, const char *cin, const char *din)
{
  if (unlabelled(tool, io->codes, "codebook", cin) || unlabelled(tool, io->data, "data", din)) return 1;
  const long noc = io->codes->num_entries;                 /* the labels of the two files, before an engine is asked for */
  int one = 1;
  for (long r = 1; r < noc; r++) one &= get_entry_label(&io->codes->rows[r]) == get_entry_label(&io->codes->rows[0]);
  if (one) { fprintf(stderr, "%s: every row of codebook %s carries one label (no other class to be wrong with)\n", tool, cin); return 1; }
  for (long s = 0; s < io->data->num_entries; s++) {
    const int l = get_entry_label(&io->data->rows[s]);
    long r = 0;
    while (r < noc && get_entry_label(&io->codes->rows[r]) != l) r++;
    if (r == noc) { fprintf(stderr, "%s: data row %ld carries label %s, which no codebook row carries\n", tool, s, find_conv_to_lab(l)); return 1; }
  }
  return 0;
}

void pak_pieces_cli(int argc, char **argv, const char *tool, long least_buffer, struct pak_pieces_cli *o)
{
  o->buffer_s = extract_parameter(argc, argv, "-buffer", OPTION);
  o->gpus_s = extract_parameter(argc, argv, "-gpus", OPTION);
  o->buffer = oatoi(o->buffer_s, 0);
  o->gpus = (int)oatoi(o->gpus_s, 1);
  if (o->buffer_s && o->buffer < least_buffer) { fprintf(stderr, "%s: -buffer %ld < %ld\n", tool, o->buffer, least_buffer); exit(1); }
  if (o->gpus < 1 || o->gpus > 64) { fprintf(stderr, "%s: -gpus %d outside 1 .. 64\n", tool, o->gpus); exit(1); }
}

float pak_linear_rate(float a, long epochs, long t) { return a * (float)(epochs - t) / (float)epochs; }
float pak_linear_radius(float r, long epochs, long t) { return 1.0f + pak_linear_rate(r - 1.0f, epochs, t); }   /* the same tree */

void pak_print_epoch_costs(FILE *fp, long epochs, float alpha, const float *eps, const double *cost, const int64_t *correct, long rows)
{
  for (long t = 0; cost && t < epochs; t++) {
    fprintf(fp, "epoch %ld alpha %.9g ", t, (double)pak_linear_rate(alpha, epochs, t));
    if (eps) fprintf(fp, "eps %.9g ", (double)pak_linear_rate(*eps, epochs, t));
    fprintf(fp, "cost %.17g accuracy %.2f %%\n", cost[t], 100.0 * (double)correct[t] / (double)rows);
  }
}
void pak_print_final_cost(FILE *fp, double cost, int64_t correct, long rows)
{
  fprintf(fp, "final cost %.17g accuracy %.2f %%\n", cost, 100.0 * (double)correct / (double)rows);
}

int pak_save_codes(struct entries *codes, const char *cout)
{
  ifverbose(2) fprintf(stderr, "Codebook entries are saved to file %s\n", cout);
  return save_entries(codes, cout) ? 1 : 0;
}
