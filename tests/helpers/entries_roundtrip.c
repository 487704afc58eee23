/* entries_roundtrip.c -- the GPU-free unit of the tools' host library (pak_io.c, linked alone with -lm) on real files:
 * made to run under AddressSanitizer / UBSan as well as plain.  For every source on the command line, then for a
 * small `gen:` source and for a file written here that has what the golden files lack (weight=, fixed=, several
 * labels, comment and blank lines, CR LF, an all-masked row), once with labels needed and once without:
 *
 *   open_entries -> save_entries_wcomments -> open_entries      the text trip
 *                -> save_entries_f32       -> open_entries      the raw fp32 trip
 *   pick_rows of a permutation and of its inverse; randomize_entry_order after init_random(7); close_entries on all.
 *
 * The fp32 trip must keep everything: dimension, topology, row count, every float's bits, every mask byte, all labels,
 * the weights and the fixed points.  The text format is "%g " per value and carries neither weight= nor fixed=
 * (write_entry, datafile.c:420-447), so after the text trip every float must have exactly the bits sscanf gives for the
 * "%g" rendering of the original -- the original's own bits wherever that rendering is exact, as in every file "%g"
 * wrote -- rows, masks and labels must be kept, weights and fixed points must be gone, and a second text trip from
 * there must keep every bit.  One line per source and pass on stdout; exit status = number of failed checks != 0.
 * Files are written into the current directory. */
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "pak.h"

static int failures = 0;
static const char *source = "";
static void fail(const char *what, long row)
{
  printf("FAILED %s: %s (row %ld)\n", source, what, row);
  failures++;
}

/* open_entries with the library's own refusal (a missing label, say) kept off stderr, which the test wants empty;
 * a sanitizer that fires in here still ends the process with a non-zero status */
static struct entries *open_quietly(const char *name, int labels_needed)
{
  fflush(stderr);
  const int keep = dup(2), null = open("/dev/null", O_WRONLY);
  dup2(null, 2);
  struct entries *e = open_entries(name, labels_needed, 1);
  fflush(stderr);
  dup2(keep, 2);
  close(keep); close(null);
  return e;
}

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float through_text(float f)                  /* what the text trip makes of one value */
{
  char tok[64];
  float g = 0;
  snprintf(tok, sizeof tok, "%g", f);
  sscanf(tok, "%f", &g);
  return g;
}

/* row rb of b against row ra of a.  text: b went through the text format since a */
static void same_row(const struct entries *a, long ra, const struct entries *b, long rb, int text)
{
  const struct data_entry *x = &a->rows[ra], *y = &b->rows[rb];
  const int dim = a->dimension;
  for (int i = 0; i < dim; i++) {
    const int mx = x->mask && x->mask[i], my = y->mask && y->mask[i];
    if (mx != my) { fail("mask byte", rb); return; }
    if (mx) continue;
    if (bits_of(y->points[i]) != bits_of(text ? through_text(x->points[i]) : x->points[i])) { fail("float bits", rb); return; }
  }
  if (y->points != b->points + rb * dim) fail("row view", rb);
  if (x->num_labs != y->num_labs) { fail("label count", rb); return; }
  for (int k = 0; k < x->num_labs; k++) if (x->labels[k] != y->labels[k]) { fail("label", rb); return; }
  if (text) {
    if (y->weight != 0 || y->fixed != NULL) fail("the text format carries no weight or fixed point", rb);
    return;
  }
  if (x->weight != y->weight || (a->weights ? a->weights[ra] : 0) != (b->weights ? b->weights[rb] : 0)) fail("weight", rb);
  if ((x->fixed != NULL) != (y->fixed != NULL)) fail("fixed point", rb);
  else if (x->fixed && (x->fixed->xfix != y->fixed->xfix || x->fixed->yfix != y->fixed->yfix)) fail("fixed point", rb);
}

static void same_entries(const struct entries *a, const struct entries *b, int text, const char *trip)
{
  if (!b) { fail(trip, -1); return; }
  if (a->dimension != b->dimension || a->topol != b->topol || a->num_entries != b->num_entries) { fail(trip, -1); return; }
  if (a->topol > TOPOL_LVQ && (a->xdim != b->xdim || a->ydim != b->ydim || a->neigh != b->neigh)) { fail(trip, -1); return; }
  if (!text && ((a->masks != NULL) != (b->masks != NULL) || (a->weights != NULL) != (b->weights != NULL) ||
                (a->fixed_xy != NULL) != (b->fixed_xy != NULL))) fail("side arrays", -1);
  if (text && (b->weights || b->fixed_xy)) fail("side arrays after the text trip", -1);
  for (long r = 0; r < a->num_entries; r++) same_row(a, r, b, r, text);
}

static uint64_t row_hash(const struct entries *e, long r)
{
  const struct data_entry *d = &e->rows[r];
  uint64_t h = 1469598103934665603ULL;
#define MIX(v) (h = (h ^ (uint64_t)(v)) * 1099511628211ULL)
  for (int i = 0; i < e->dimension; i++) { MIX(d->mask && d->mask[i] ? 0x100000000ULL : bits_of(d->points[i])); }
  for (int k = 0; k < d->num_labs; k++) MIX(d->labels[k]);
  MIX(d->weight);
  if (d->fixed) { MIX(d->fixed->xfix); MIX(d->fixed->yfix); }
#undef MIX
  return h;
}

static void one_pass(const char *name, int labels_needed)
{
  struct entries *a = open_quietly(name, labels_needed);
  if (!a) { printf("%s labels_needed %d: not opened\n", source, labels_needed); return; }
  const long n = a->num_entries;
  long labels = 0, masked = 0, weighted = 0, fixed = 0;
  for (long r = 0; r < n; r++) {
    labels += a->rows[r].num_labs; masked += a->rows[r].mask != NULL;
    weighted += a->rows[r].weight != 0; fixed += a->rows[r].fixed != NULL;
  }

  if (save_entries_wcomments(a, "trip.txt", "#round trip\n#second comment line\n")) fail("save_entries_wcomments", -1);
  struct entries *b = open_quietly("trip.txt", labels_needed);
  same_entries(a, b, 1, "text trip");
  if (b) {
    if (save_entries_wcomments(b, "trip2.txt", NULL)) fail("save_entries_wcomments", -1);
    struct entries *c = open_quietly("trip2.txt", labels_needed);
    same_entries(b, c, 0, "second text trip");
    close_entries(c);
  }
  if (save_entries_f32(a, "trip.bin")) fail("save_entries_f32", -1);
  struct entries *f = open_quietly("trip.bin", labels_needed);
  same_entries(a, f, 0, "fp32 trip");

  long *perm = malloc(sizeof(long) * (n + 1)), *inv = malloc(sizeof(long) * (n + 1));
  for (long k = 0; k < n; k++) { perm[k] = (k * 7 + 3) % n; }             /* a permutation when 7 does not divide n ... */
  if (n % 7 == 0) for (long k = 0; k < n; k++) perm[k] = n - 1 - k;       /* ... the reversal otherwise */
  for (long k = 0; k < n; k++) inv[perm[k]] = k;
  struct entries *p = pick_rows(a, perm, n), *q = pick_rows(p, inv, n);
  for (long k = 0; k < n; k++) same_row(a, perm[k], p, k, 0);
  same_entries(a, q, 0, "pick_rows of the inverse permutation");

  uint64_t sum = 0, order = 0, sum2 = 0;
  for (long r = 0; r < n; r++) sum += row_hash(p, r);
  init_random(7);
  randomize_entry_order(p);
  for (long r = 0; r < n; r++) {
    sum2 += row_hash(p, r); order = order * 31 + row_hash(p, r);
    if (p->rows[r].points != p->points + r * p->dimension) { fail("row view after the shuffle", r); break; }
  }
  if (p->num_entries != n || sum != sum2) fail("the shuffle does not permute the rows", -1);

  printf("%s labels_needed %d: dim %d topol %d %dx%d neigh %d rows %ld labels %ld masked %ld weighted %ld fixed %ld order %016llx\n",
         source, labels_needed, a->dimension, a->topol, a->xdim, a->ydim, a->neigh, n, labels, masked, weighted, fixed,
         (unsigned long long)order);
  free(perm); free(inv);
  close_entries(a); close_entries(b); close_entries(f); close_entries(p); close_entries(q);
}

static void one_source(const char *name)
{
  const char *slash = strrchr(name, '/');
  source = slash ? slash + 1 : name;
  one_pass(name, 1);
  one_pass(name, 0);
}

int main(int argc, char **argv)
{
  for (int i = 1; i < argc; i++) one_source(argv[i]);
  one_source("gen:k=3,dim=5,n=40,seed=9,labels=1");
  FILE *fp = fopen("made_here.dat", "w");
  if (!fp) { perror("made_here.dat"); return 1; }
  fputs("# a comment before the header\n3 rect 3 2 gaussian\n# and one after it\n"
        "1 2.5 -3e-3 A B weight=3\n\n"
        "x 0.1 x B fixed=2,1\r\n"
        "x x x C\n"
        "   \t\n"
        "16777217 1e-7 .5 C A A weight=-2 fixed=0,0\n"
        "1.00000005960464477539 +4 -0 D\n"
        "7 8 x E fixed=1,1\n"
        "9 10 11 F", fp);
  fclose(fp);
  one_source("made_here.dat");
  printf("failed checks %d\n", failures);
  return failures != 0;
}
