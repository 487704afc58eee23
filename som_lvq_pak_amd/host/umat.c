/* umat -- the U-matrix picture of a trained map as an EPS / PS file (SOM_PAK umat.c, map.c): same flags, same output
 * outside the PostScript prologue, byte for byte.  The distances between neighbouring model vectors, the medians at the
 * units' own positions, the scaling and the optional filters come from the MI355X engine (somhip_umatrix); the host
 * lays the page out (umat.c:344-493) and prints grey levels and labels (umat.c:528-677).  The prologue is this project's
 * own (umat_prologue.h); -headerfile or UMAT_HEADERFILE puts any other in its place. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <time.h>
#include "pak.h"
#include "umat_prologue.h"

static const char *usage =
    "umat - EPS/PS picture of the U-matrix of a map (MI355X engine)\n"
    "Required parameters:\n"
    "  -cin filename         input codebook file (a hexa or rect map)\n"
    "Optional parameters:\n"
    "  -o filename           output file (default: standard output); .ps / .eps selects the mode\n"
    "  -eps | -ps            EPS picture (the default) or a PS page\n"
    "  -portrait | -landscape   orientation of the PS page (default: by the map's shape)\n"
    "  -paper A4|A3          paper of the PS page (default A4)\n"
    "  -border               outline the blocks\n"
    "  -onlylabs | -nolabs   labels only / no labels\n"
    "  -W float  -B float    white and black threshold (default 1.0 and 0.0)\n"
    "  -title string | -notitle   title of the PS page (default: the codebook's name)\n"
    "  -font name  -fontsize float   label font, size relative to the radius of a unit\n"
    "  -average  -median     filter the matrix (the average runs first)\n"
    "  -headerfile filename  PostScript prologue to use instead of the built-in one (also: UMAT_HEADERFILE)\n"
    "  -swapx  -swapy        mirror the picture\n"
    "  -v level              2: smallest and largest distance between neighbouring units\n";

struct paper { const char *name; int width, height; };
static const struct paper papers[] = {{"A4", 595, 841}, {"A3", 841, 1190}, {NULL, 0, 0}};
#define MARGIN 36

struct layout { float width, height, xstep, ystep, radius, x0, y0; };

struct options {
  int ps, orientation;                       /* orientation: 0 by shape, 1 portrait, 2 landscape */
  const struct paper *paper;
  int border, blocks, labels, notitle, swapx, swapy;
  float wt, bt, fontsize;
  const char *font, *title, *headerfile;
};

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

static const char *date_line(void)
{
  time_t now = time(NULL);
  return ps_escaped(ctime(&now));
}

static int mode_of_suffix(const char *name)      /* 1 ps, 2 eps, 0 unknown */
{
  const char *dot = name ? strrchr(name, '.') : NULL;
  if (!dot) return 0;
  if (strcasecmp(dot + 1, "ps") == 0) return 1;
  if (strcasecmp(dot + 1, "eps") == 0) return 2;
  return 0;
}

/* the picture is 1000 wide; steps, radius and height follow from the matrix (umat.c:460-493), float by float */
static void lay_out(struct layout *l, int topol, int ux, int uy)
{
  l->width = 1000;
  if (topol == TOPOL_RECT) {
    l->xstep = l->width / (float)ux;
    l->ystep = l->xstep;
    l->height = uy * l->ystep;
    l->x0 = l->xstep * 0.5;
    l->y0 = l->ystep * 0.5;
    l->radius = l->xstep * 0.5;
  } else {
    l->xstep = l->width / (float)(ux + 1);
    l->ystep = l->xstep * sqrt(3) * 0.5;
    l->radius = l->xstep / sqrt(3);
    l->height = (uy - 1) * l->ystep + 2.0 * l->radius;
    l->x0 = l->xstep * 0.5;
    l->y0 = l->radius;
  }
}

static int write_prologue(FILE *fp, const char *headerfile)
{
  if (!headerfile) {
    for (int i = 0; umat_prologue[i]; i++) fputs(umat_prologue[i], fp);
    return 0;
  }
  FILE *h = fopen(headerfile, "r");
  if (!h) { fprintf(stderr, "umat: can't read PS header file %s\n", headerfile); return 1; }
  for (int c; (c = fgetc(h)) != EOF;) fputc(c, fp);
  fclose(h);
  return 0;
}

/* the EPS object, umat.c:528-677 */
static int write_eps(FILE *fp, struct entries *codes, const float *u, const struct layout *l, const struct options *o)
{
  const int hexa = codes->topol == TOPOL_HEXA;
  const char *block = hexa ? "H" : "R", *start = hexa ? "XSH" : "XSR";
  const int mx = codes->xdim, my = codes->ydim, ux = 2 * mx - 1, uy = 2 * my - 1;
  fprintf(fp, "%%!PS-Adobe-3.0 EPSF-3.0\n");
  fprintf(fp, "%%%%BoundingBox: 0 0 %d %d\n", (int)ceil(l->width), (int)ceil(l->height));
  fprintf(fp, "%%%%Title: %s\n%%%%Creator: umat V1.1\n", ps_escaped(o->title));
  fprintf(fp, "%%%%CreationDate: %s", date_line());
  fprintf(fp, "%%%%Pages: 0\n");
  fprintf(fp, "%%%%DocumentFonts: %s\n%%%%DocumentNeededFonts: %s\n", o->font, o->font);
  fprintf(fp, "%%%%EndComments\n");
  if (write_prologue(fp, o->headerfile)) return 1;
  fprintf(fp, "/radius %f def\n/xstep %f def\n/ystep %f def\n", l->radius, l->xstep, l->ystep);
  fprintf(fp, "/picwidth %f def /picheight %f def\n", l->width, l->height);
  fprintf(fp, "%%%%IncludeFont: %s\n", o->font);
  fprintf(fp, "/fontname /%s def\n", o->font);
  if (o->fontsize > 0.0) fprintf(fp, "/fontsize %f def\n", o->fontsize);
  fprintf(fp, "selfont\n");
  fprintf(fp, "/doborder %s def\n", o->border ? "true" : "false");
  fprintf(fp, "/wt %f def /bt %f def\n", o->wt, o->bt);
  fprintf(fp, "/xoffset %f def /yoffset %f def\n", l->x0, (l->height - l->y0));
  if (o->swapx) fprintf(fp, "swapx\n");
  if (o->swapy) fprintf(fp, "swapy\n");
  fprintf(fp, "/y 0 def\n/xoff xoffset def\n/yoff yoffset def\n");
  if (o->blocks)
    for (int y = 0; y < uy; y++) {
      fprintf(fp, "%s ", start);
      for (int x = 0; x < ux; x++) fprintf(fp, "%d %s ", (int)(100 * u[(size_t)y * ux + x]), block);
      fprintf(fp, "NL\n");
    }
  fprintf(fp, "/y 0 def\n/xoff xoffset def\n/yoff yoffset def\n");
  if (o->labels)
    for (int y = 0; y < my; y++) {
      fprintf(fp, "%s ", start);
      for (int x = 0; x < mx; x++) {
        const struct data_entry *d = &codes->rows[(long)y * mx + x];
        float color = o->blocks ? u[(size_t)(2 * y) * ux + 2 * x] * 100 : 100;
        int numlabs = d->num_labs;
        if (numlabs == 1)
          fprintf(fp, "(%s) %d LAB ", ps_escaped(find_conv_to_lab(d->labels[0])), (int)color);
        else if (numlabs > 1) {
          for (int i = 0; i < d->num_labs; i++) {
            if (d->labels[i] == LABEL_EMPTY) { numlabs = i; break; }
            fprintf(fp, "(%s) ", ps_escaped(find_conv_to_lab(d->labels[i])));
          }
          fprintf(fp, "%d %d ML ", numlabs, (int)color);
        } else
          fprintf(fp, "%d LN ", (int)color);
      }
      fprintf(fp, "NL NL\n");                      /* labels sit on every other row of the matrix */
    }
  fprintf(fp, "end\n");
  fprintf(fp, "%% end of EPS object\n");
  return 0;
}

/* the PS page around it, umat.c:344-405: margins of 36 points, the picture scaled to fit and centred */
static int write_page(FILE *fp, struct entries *codes, const float *u, const struct layout *l, const struct options *o,
                      int landscape)
{
  int w = l->width, h = l->height;
  const int titled = o->title && !o->notitle;
  if (titled) w += 24;
  int pw = o->paper->width - 2 * MARGIN, ph = o->paper->height - 2 * MARGIN;
  fprintf(fp, "%%!PS-Adobe-2.0\n%%%%Pages: 1\n");
  fprintf(fp, "%%%%Creator: umat V1.1\n");
  fprintf(fp, "%%%%CreationDate: %s", date_line());
  if (landscape) {
    fprintf(fp, "%d %d translate 90 rotate\n", MARGIN + pw, MARGIN);
    int t = pw; pw = ph; ph = t;
  } else
    fprintf(fp, "%d %d translate\n", MARGIN, MARGIN);
  const float s1 = (float)pw / (float)w, s2 = (float)ph / (float)h;
  const float scale = s1 < s2 ? s1 : s2;
  const int xs = (pw - scale * w) * 0.5, ys = (ph - scale * h) * 0.5;
  fprintf(fp, "gsave %d %d translate %f dup scale\n", xs, ys, scale);
  if (titled) {
    fprintf(fp, "gsave /Helvetica findfont 18 scalefont setfont\n");
    fprintf(fp, "0 setgray %f %f 8 add moveto\n", (float)2.0, l->height);
    fprintf(fp, "(%s - Dim: %d, Size: %d*%d units, %s neighborhood) show\n", ps_escaped(o->title), codes->dimension,
            codes->xdim, codes->ydim, codes->neigh == NEIGH_GAUSSIAN ? "gaussian" : "bubble");
    fprintf(fp, "grestore\n");
  }
  if (write_eps(fp, codes, u, l, o)) return 1;
  fprintf(fp, "grestore\nshowpage\n");
  return 0;
}

int main(int argc, char **argv)
{
  struct options o;
  memset(&o, 0, sizeof o);
  char *s;
  global_options(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  o.paper = &papers[0];
  o.border = extract_parameter(argc, argv, "-border", OPTION2) != NULL;
  if (extract_parameter(argc, argv, "-portrait", OPTION2)) o.orientation = 1;
  if (extract_parameter(argc, argv, "-landscape", OPTION2)) o.orientation = 2;
  int mode = 0;
  if (extract_parameter(argc, argv, "-ps", OPTION2)) mode = 1;
  if (extract_parameter(argc, argv, "-eps", OPTION2)) mode = 2;
  o.wt = oatof(extract_parameter(argc, argv, "-W", OPTION), 1.0);
  o.bt = oatof(extract_parameter(argc, argv, "-B", OPTION), 0.0);
  char *out_name = extract_parameter(argc, argv, "-o", OPTION);
  if (mode == 0) mode = mode_of_suffix(out_name);
  o.font = (s = extract_parameter(argc, argv, "-font", OPTION)) ? s : "Helvetica";
  o.fontsize = oatof(extract_parameter(argc, argv, "-fontsize", OPTION), -1.0);
  o.title = extract_parameter(argc, argv, "-title", OPTION);
  o.notitle = extract_parameter(argc, argv, "-notitle", OPTION2) != NULL;
  if ((s = extract_parameter(argc, argv, "-paper", OPTION))) {
    const struct paper *p = papers;
    while (p->name && strcasecmp(p->name, s) != 0) p++;
    if (!p->name) { fprintf(stderr, "Unknown paper type: %s\n", s); exit(1); }
    o.paper = p;
  }
  int filters = 0;
  if (extract_parameter(argc, argv, "-average", OPTION2)) filters |= SOMHIP_UMAT_AVERAGE;
  if (extract_parameter(argc, argv, "-median", OPTION2)) filters |= SOMHIP_UMAT_MEDIAN;
  o.blocks = extract_parameter(argc, argv, "-onlylabs", OPTION2) == NULL;
  o.labels = extract_parameter(argc, argv, "-nolabs", OPTION2) == NULL;
  o.swapx = extract_parameter(argc, argv, "-swapx", OPTION2) != NULL;
  o.swapy = extract_parameter(argc, argv, "-swapy", OPTION2) != NULL;
  char *in_name = extract_parameter(argc, argv, "-cin", ALWAYS);
  if ((s = getenv("UMAT_HEADERFILE"))) o.headerfile = s;
  if ((s = extract_parameter(argc, argv, "-headerfile", OPTION))) o.headerfile = s;

  struct entries *codes = open_entries(in_name, 0, 1);
  if (!codes) { fprintf(stderr, "Can't open code file %s\nCan't load file\n", in_name); return 1; }
  if (codes->topol != TOPOL_HEXA && codes->topol != TOPOL_RECT) {
    fprintf(stderr, "umat: file %s is not a map file: only hexa and rect maps have a U-matrix\n", in_name);
    return 1;
  }
  if (codes->masks) {
    fprintf(stderr, "umat: codebook %s has masked components (x); the U-matrix of masked codebooks is not supported\n", in_name);
    return 1;
  }
  if (codes->num_entries != (long)codes->xdim * codes->ydim) {
    fprintf(stderr, "umat: codebook %s has %ld entries, its %d x %d map needs %ld\n", in_name, codes->num_entries,
            codes->xdim, codes->ydim, (long)codes->xdim * codes->ydim);
    return 1;
  }
  if (codes->xdim < 2 || codes->ydim < 2) {
    fprintf(stderr, "umat: a %d x %d map has no U-matrix (both sides must be at least 2)\n", codes->xdim, codes->ydim);
    return 1;
  }

  const int ux = 2 * codes->xdim - 1, uy = 2 * codes->ydim - 1;
  float *u = malloc(sizeof(float) * (size_t)ux * uy);
  double minmax[2];
  somhip_engine *en = NULL;
  somhip_codebook *cb = NULL;
  if (somhip_engine_create(0, &en)) { fprintf(stderr, "%s\n", somhip_last_error()); return 1; }
  if (somhip_codebook_create(en, codes->points, NULL, codes->num_entries, codes->dimension, codes->topol, codes->neigh,
                             codes->xdim, codes->ydim, 0, codes->num_entries, &cb) ||
      somhip_umatrix(cb, filters, u, minmax)) {
    fprintf(stderr, "%s\n", somhip_last_error());
    return 1;
  }
  ifverbose(2) {
    fprintf(stderr, "minimum distance between elements : %f\n", minmax[0]);
    fprintf(stderr, "maximum distance between elements : %f\n", minmax[1]);
  }

  if (mode == 0) mode = 2;
  if (!o.title) o.title = in_name;
  const int landscape = o.orientation ? o.orientation == 2 : codes->xdim >= codes->ydim;
  FILE *fp = out_name ? fopen(out_name, "w") : stdout;
  if (!fp) { fprintf(stderr, "can't open output file\n"); return 1; }
  struct layout l;
  lay_out(&l, codes->topol, ux, uy);
  const int rc = mode == 2 ? write_eps(fp, codes, u, &l, &o) : write_page(fp, codes, u, &l, &o, landscape);
  if (out_name) fclose(fp);
  free(u);
  somhip_codebook_destroy(cb);
  close_entries(codes);
  somhip_engine_destroy(en);
  return rc;
}
