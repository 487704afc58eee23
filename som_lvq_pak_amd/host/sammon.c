/* sammon -- Sammon mapping of a codebook into the plane (SOM_PAK sammon.c): same flags, files, messages and bits.
 * The pair distances and the iteration run on the MI355X engine (somhip_sammon_zero_pairs, somhip_sammon); the host
 * replays remove_identicals' list walk over the zero-distance pairs (sammon.c:84-128), draws the initial table from
 * orand, and writes the 2-dim codebook and the PostScript picture (sammon.c:276-420). */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "sammon - generates a Sammon mapping from a given list (MI355X engine)\n"
    "Required parameters:\n"
    "  -cin filename         input codebook file\n"
    "  -cout filename        output codebook filename\n"
    "  -rlen integer         running length\n"
    "Optional parameters:\n"
    "  -eps                  produce an EPS picture of map\n"
    "  -ps                   produce an PS picture of map\n"
    "  -rand integer         seed for random number generator. 0 is current time\n"
    "  -buffer integer       accepted, unused\n"
    "  -v level              2: mapping error after every iteration\n";

/* the zero-distance pairs of the codebook, sorted by (i, j); NULL on failure */
static uint32_t *zero_pairs(somhip_codebook *cb, long noc, int64_t *n_pairs)
{
  int64_t cap = 16 * (int64_t)noc;
  uint32_t *pairs = malloc(sizeof(uint32_t) * 2 * cap);
  if (somhip_sammon_zero_pairs(cb, pairs, cap, n_pairs)) { fprintf(stderr, "%s\n", somhip_last_error()); free(pairs); return NULL; }
  if (*n_pairs > cap) {                                 /* many identical rows: once more with room for all */
    if (*n_pairs > ((int64_t)1 << 28)) {
      fprintf(stderr, "sammon: %lld pairs of identical entries in the codebook are more than this tool lists\n", (long long)*n_pairs);
      free(pairs);
      return NULL;
    }
    cap = *n_pairs;
    free(pairs);
    pairs = malloc(sizeof(uint32_t) * 2 * cap);
    if (somhip_sammon_zero_pairs(cb, pairs, cap, n_pairs)) { fprintf(stderr, "%s\n", somhip_last_error()); free(pairs); return NULL; }
  }
  return pairs;
}

/* remove_identicals (sammon.c:84-128) over the reported pairs: the reference walks its list and, for every entry still
 * there, drops each later entry at distance 0 -- with the computed distance, which is not transitive, so the walk
 * itself is replayed.  Its counters: ii counts the outer entries from 1; ij starts at ii + 1 and advances by two after
 * a removal, by one otherwise (sammon.c:103-121).  Rows without a live partner need no walk.  Returns the number of
 * rows left; gone[r] = 1 for the removed ones. */
static long remove_identicals(long noc, const uint32_t *pairs, int64_t n_pairs, char *gone)
{
  long *next = malloc(sizeof(long) * (noc + 1));
  int64_t *first = malloc(sizeof(int64_t) * (noc + 1));
  for (long r = 0; r < noc; r++) next[r] = r + 1 < noc ? r + 1 : -1;
  int64_t t = 0;
  for (long r = 0; r <= noc; r++) {
    while (t < n_pairs && (long)pairs[2 * t] < r) t++;
    first[r] = t;
  }
  long left = noc, ii = 1;
  for (long i = 0; i != -1; i = next[i], ii++) {
    int live = 0;
    for (int64_t p = first[i]; p < first[i + 1]; p++) live |= !gone[pairs[2 * p + 1]];
    if (!live) continue;
    long ij = ii + 1, prev = i;
    int64_t p = first[i];
    for (long q = next[i]; q != -1;) {
      while (p < first[i + 1] && (long)pairs[2 * p + 1] < q) p++;
      if (p < first[i + 1] && (long)pairs[2 * p + 1] == q) {
        fprintf(stderr, "Identical entries in codebook ");
        fprintf(stderr, "(entries %ld, %ld), removing one.\n", ii, ij);
        gone[q] = 1;
        left--;
        next[prev] = next[q];
        q = next[q];
        ij += 2;
      } else {
        prev = q;
        q = next[q];
        ij++;
      }
    }
  }
  free(next); free(first);
  return left;
}

/* drop the removed rows from the entries in place */
static void compact_entries(struct entries *codes, const char *gone)
{
  int dim = codes->dimension;
  long m = 0;
  for (long r = 0; r < codes->num_entries; r++) {
    if (gone[r]) { free(codes->rows[r].labels); continue; }
    if (m != r) {
      memmove(codes->points + m * dim, codes->points + r * dim, sizeof(float) * dim);
      codes->rows[m] = codes->rows[r];
    }
    codes->rows[m].points = codes->points + m * dim;
    m++;
  }
  codes->num_entries = m;
}

static const char *ps_escaped(const char *text)       /* ( ) and \ get a backslash in a PostScript string */
{
  static char buf[2050];
  size_t n = 0;
  for (; text && *text && n < sizeof buf - 2; text++) {
    if (*text == '(' || *text == ')' || *text == '\\') buf[n++] = '\\';
    buf[n++] = *text;
  }
  buf[n] = 0;
  return buf;
}

/* <base>_sa.eps / <base>_sa.ps as sammon.c:276-420 writes it: points shifted to the lower left corner, a dot (and the
 * first label) per row and, when `lines`, the map's grid.  The reference starts its maxima at FLT_MIN (:288-290) and
 * decides the scale in double (:316-319); both are kept. */
static void save_picture(struct entries *map, const char *base, int ps, int lines)
{
  char name[4096];
  snprintf(name, sizeof name, "%s_sa.%s", base, ps ? "ps" : "eps");
  FILE *fp = fopen(name, "w");
  if (!fp) { printf("Can't open file%s\n", name); return; }
  long n = map->num_entries;
  float xmi = FLT_MAX, xma = FLT_MIN, ymi = FLT_MAX, yma = FLT_MIN, frac;
  for (long r = 0; r < n; r++) {
    const float *p = map->rows[r].points;
    if (xmi > p[0]) xmi = p[0];
    if (xma < p[0]) xma = p[0];
    if (ymi > p[1]) ymi = p[1];
    if (yma < p[1]) yma = p[1];
  }
  if ((xma - xmi) * 1.5 > (yma - ymi)) frac = 510.0 / (xma - xmi);
  else frac = 760.0 / (yma - ymi);
  for (long r = 0; r < n; r++) {
    float *p = map->rows[r].points;
    p[0] = p[0] - xmi;
    p[1] = p[1] - ymi;
  }
  fprintf(fp, "%%!PS-Adobe-2.0 EPSF-2.0\n%%%%Title: %s\n%%%%Creator: sammon\n", "undefined");
  if (ps) {
    fprintf(fp, "%%%%Pages: 1\n%%%%EndComments\n40 40 translate\n");
    fprintf(fp, "/gscale %f def\ngscale dup scale\n", frac);
  } else {
    fprintf(fp, "%%%%BoundingBox: 0 0 %f %f\n", xma - xmi, yma - ymi);
    fprintf(fp, "%%%%Pages: 0\n%%%%EndComments\n/gscale %f def\n", frac);
  }
  fprintf(fp, "/Helvetica findfont 12 gscale div scalefont setfont\n");
  fprintf(fp, "/radius %f def\n", 2.0 / frac);
  fputs("/LN\n{newpath\nradius 0 360 arc fill\n} def\n/LP\n{dup stringwidth pop\n-2 div 0 rmoveto show} def\n", fp);
  fprintf(fp, "%f setlinewidth\n0 setgray\n", 0.2 / frac);
  for (long r = 0; r < n; r++) {
    struct data_entry *d = &map->rows[r];
    fprintf(fp, "%f %f LN\n", d->points[0], d->points[1]);
    if (get_entry_label(d) != LABEL_EMPTY) {
      fprintf(fp, "%f %f moveto\n", d->points[0], d->points[1]);
      fprintf(fp, "(%s) LP\n", ps_escaped(find_conv_to_lab(get_entry_label(d))));
    }
  }
  if (lines) {
    /* the reference walks its list with a column counter (:370-413): row t is column t % xdim of lattice row t / xdim */
    int xdim = map->xdim, ydim = map->ydim;
    for (int along = 1; along >= 0; along--)                /* first the lattice rows, then column after column */
      for (int col = 0; col < (along ? 1 : xdim); col++)
        for (long t = along ? 0 : col; t < n; t += along ? 1 : xdim) {
          const float *p = map->rows[t].points;
          long step = along ? t % xdim : t / xdim, last = along ? xdim - 1 : ydim - 1;
          if (step == 0) fprintf(fp, "newpath\n%f %f moveto\n", p[0], p[1]);
          else {
            fprintf(fp, "%f %f lineto\n", p[0], p[1]);
            if (step == last) fprintf(fp, "stroke\n");
          }
        }
  }
  if (ps) fprintf(fp, "showpage\n");
  fclose(fp);
}

int main(int argc, char **argv)
{
  global_options(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *in_code_file = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *out_code_file = extract_parameter(argc, argv, "-cout", ALWAYS);
  long length = oatoi(extract_parameter(argc, argv, "-rlen", ALWAYS), 1);
  long randomize = oatoi(extract_parameter(argc, argv, "-rand", OPTION), 0);
  int eps = extract_parameter(argc, argv, "-eps", OPTION2) != NULL;
  int ps = extract_parameter(argc, argv, "-ps", OPTION2) != NULL;
  (void)extract_parameter(argc, argv, "-buffer", OPTION);

  ifverbose(2) fprintf(stderr, "Code entries from file %s\n", in_code_file);
  struct entries *codes = open_entries(in_code_file, 0, 1);
  if (!codes) { fprintf(stderr, "can't open code file %s\n", in_code_file); return 1; }
  if (codes->masks) {
    fprintf(stderr, "sammon: codebook %s has masked components (x); the Sammon mapping of masked codebooks is not supported\n", in_code_file);
    return 1;
  }
  if (length < 0) length = 0;
  init_random((int)randomize);

  somhip_engine *en = NULL;
  somhip_codebook *cb = NULL;
  if (somhip_engine_create(0, &en)) { fprintf(stderr, "%s\n", somhip_last_error()); return 1; }
  /* the mapping looks at the rows as a list: no lattice on the device (a map file may hold any number of rows here) */
  if (somhip_codebook_create(en, codes->points, NULL, codes->num_entries, codes->dimension, TOPOL_LVQ, 0, 0, 0, 0,
                             codes->num_entries, &cb)) { fprintf(stderr, "%s\n", somhip_last_error()); return 1; }

  /* remove identical entries from the codebook */
  long noc = codes->num_entries;
  int64_t n_pairs = 0;
  uint32_t *pairs = zero_pairs(cb, noc, &n_pairs);
  if (!pairs) return 1;
  int removed = 0;
  if (n_pairs > 0) {
    char *gone = calloc(noc + 1, 1);
    long left = remove_identicals(noc, pairs, n_pairs, gone);
    removed = left != noc;
    compact_entries(codes, gone);
    free(gone);
    noc = codes->num_entries;
    somhip_codebook_destroy(cb);
    cb = NULL;
    if (noc >= 1 && somhip_codebook_create(en, codes->points, NULL, noc, codes->dimension, TOPOL_LVQ, 0, 0, 0, 0, noc, &cb)) {
      fprintf(stderr, "%s\n", somhip_last_error());
      return 1;
    }
  }
  free(pairs);
  ifverbose(3) fprintf(stderr, "%ld entries in codebook\n", noc);
  if (noc < 2) {
    fprintf(stderr, "sammon: %ld entry left in the codebook: nothing to map\n", noc);
    return 1;
  }

  /* the initial table, sammon.c:164-167 */
  float *x = malloc(sizeof(float) * noc), *y = malloc(sizeof(float) * noc);
  for (long i = 0; i < noc; i++) {
    x[i] = (float)(orand() % noc) / noc;
    y[i] = (float)(i) / noc;
  }
  double *err = verbose_level >= 2 && length > 0 ? malloc(sizeof(double) * length) : NULL;
  if (somhip_sammon(cb, length, x, y, err)) { fprintf(stderr, "%s\n", somhip_last_error()); return 1; }
  for (long i = 0; err && i < length; i++) fprintf(stdout, "Mapping error: %7.3f\n", (float)err[i]);

  struct entries *spics = calloc(1, sizeof *spics);
  spics->dimension = 2; spics->topol = codes->topol; spics->neigh = codes->neigh;
  spics->xdim = codes->xdim; spics->ydim = codes->ydim; spics->num_entries = noc;
  spics->points = malloc(sizeof(float) * 2 * (noc + 1));
  spics->rows = calloc(noc + 1, sizeof(struct data_entry));
  for (long i = 0; i < noc; i++) {
    float *p = spics->points + 2 * i;
    spics->rows[i].points = p;
    p[0] = x[i];
    p[1] = y[i];
    for (int k = 0; k < codes->rows[i].num_labs; k++) add_entry_label(spics, i, codes->rows[i].labels[k]);
  }
  ifverbose(2) fprintf(stderr, "Save code entries to file %s\n", out_code_file);
  if (save_entries(spics, out_code_file)) return 1;

  char *base_name = strdup(out_code_file);
  char *dot = strrchr(base_name, '.');
  if (dot) *dot = '\0';
  /* no grid lines when the file is not a map file, or when rows were removed */
  if (codes->topol != TOPOL_RECT && codes->topol != TOPOL_HEXA) removed = 1;
  if (ps || eps) save_picture(spics, base_name, ps, !removed);

  free(base_name); free(x); free(y); free(err);
  somhip_codebook_destroy(cb);
  close_entries(codes);
  close_entries(spics);
  somhip_engine_destroy(en);
  return 0;
}
