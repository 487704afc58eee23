/* planes -- component planes of a map, and the trajectory of a data file over it, as EPS / PS files (SOM_PAK planes.c):
 * same flags, same file names, same output byte for byte outside the bodies of the two procedure definitions (/LN, /LP),
 * which are this project's own wording of the same operators.  The grey levels of every plane come from the MI355X
 * engine (somhip_planes: the rows are read where they lie, plane by plane in windows), the winners of the trajectory
 * from somhip_find_winners; the host lays the units out and prints. */
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include "pak.h"

static const char *usage =
    "planes - EPS/PS pictures of the component planes of a map (MI355X engine)\n"
    "Required parameters:\n"
    "  -cin filename         input codebook file (a hexa or rect map); output goes beside it:\n"
    "                        <name without its last suffix>_p<k>.eps per plane, _tr.eps for the trajectory\n"
    "Optional parameters:\n"
    "  -din filename         input data: draw the path of its best-matching units (.dat, raw fp32 or gen:)\n"
    "  -plane integer        component to draw, counted from 1 (default 1; 0 = all of them)\n"
    "  -ps integer           1: PS pages (.ps) instead of EPS pictures\n"
    "  -buffer integer       accepted; the data is read at once\n"
    "  -selfuncs name        select a set of functions\n"
    "  -v level              2: name the files as they are read\n";

#define XSTEP 40
#define SLAB_BYTES (64l << 20)             /* grey levels held at once by either side under -plane 0 */

struct picture { int ps, xdim, ydim, ystep, offset, xsize, ysize; };

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

static FILE *open_picture(const char *base, const char *tail, const struct picture *pic)
{
  size_t len = strlen(base) + strlen(tail) + 8;
  char *name = malloc(len);
  snprintf(name, len, "%s%s.%s", base, tail, pic->ps ? "ps" : "eps");
  FILE *fp = fopen(name, "w");
  if (!fp) fprintf(stderr, "planes: can't write %s\n", name);
  free(name);
  if (!fp) return NULL;
  fprintf(fp, "%%!PS-Adobe-2.0 EPSF-2.0\n%%%%Title: undefined\n%%%%Creator: planes\n");
  if (pic->ps) {
    fprintf(fp, "%%%%Pages: 1\n%%%%EndComments\n550 40 translate\n90 rotate\n");
    fprintf(fp, "760 %d div 510 %d div lt\n", pic->xsize, pic->ysize);
    fprintf(fp, "   {760 %d 0 sub div} {510 %d div} ifelse\n", pic->xsize, pic->ysize);
    fprintf(fp, "/gscale exch def\ngscale dup scale\n");
  } else {
    fprintf(fp, "%%%%BoundingBox: 0 0 %d %d\n", pic->xsize, pic->ysize);
    fprintf(fp, "%%%%Pages: 0\n%%%%EndComments\n");
  }
  return fp;
}

static void unit_position(const struct picture *pic, long k, int *xp, int *yp)
{
  *xp = XSTEP * (int)(k % pic->xdim) + XSTEP / 2;
  *yp = pic->ystep * (int)(k / pic->xdim) + pic->ystep / 2;
  if ((k / pic->xdim) % 2) *xp += pic->offset;
}

/* one plane: a disc per unit in list order, then the units' first labels (planes.c:93-218) */
static int write_plane(const char *base, const struct picture *pic, struct entries *codes, int plane, const float *grey)
{
  char tail[32];
  snprintf(tail, sizeof tail, "_p%d", plane + 1);
  FILE *fp = open_picture(base, tail, pic);
  if (!fp) return 1;
  int xp, yp;
  fprintf(fp, "/fontsize %d def\n", (int)(XSTEP / 3));
  fprintf(fp, "0 %d translate\n1 -1 scale\n", pic->ysize);
  fprintf(fp, "/radius %d def\n", (int)(XSTEP / 2.2));
  fputs("/LN\n"
        "{ % x y grey LN: a disc of that grey around (x, y)\n"
        "  setgray newpath radius 0 360 arc closepath fill\n"
        "} def\n", fp);
  for (long k = 0; k < codes->num_entries; k++) {
    unit_position(pic, k, &xp, &yp);
    fprintf(fp, "%d %d %f LN\n", xp, yp, grey[k]);
  }
  fprintf(fp, "0 setgray\n/Helvetica findfont fontsize scalefont setfont\n");
  fputs("/LP\n"
        "{ % (label) LP: the label centred on the current point, upright although the picture's y axis points down\n"
        "  gsave currentpoint translate 1 -1 scale\n"
        "  dup stringwidth pop 2 div neg 0 moveto show\n"
        "  grestore\n"
        "} def\n", fp);
  for (long k = 0; k < codes->num_entries; k++) {
    int label = get_entry_label(&codes->rows[k]);
    if (label == LABEL_EMPTY) continue;
    unit_position(pic, k, &xp, &yp);
    fprintf(fp, "%d %d moveto (%s) LP\n", xp, yp, ps_escaped(find_conv_to_lab(label)));
  }
  if (pic->ps) fprintf(fp, "showpage\n");
  return fclose(fp) != 0;
}

/* the trajectory: a circle per unit (x outermost), then one path per run of rows that have a winner; a row with every
 * component masked (ret 0) or without a winner (index < 0) ends the path (planes.c:270-398) */
static int write_trajectory(const char *base, const struct picture *pic, long n, const int32_t *idx, const int32_t *ret)
{
  FILE *fp = open_picture(base, "_tr", pic);
  if (!fp) return 1;
  int xp, yp;
  fprintf(fp, "0 %d translate\n1 -1 scale\n", pic->ysize);
  fprintf(fp, "1 setlinewidth\n0.8 setgray\n/radius %d def\n", (int)(XSTEP / 2.2));
  fputs("/LN\n"
        "{ % x y LN: the outline of a unit around (x, y)\n"
        "  newpath radius 0 360 arc closepath stroke\n"
        "} def\n", fp);
  for (int i = 0; i < pic->xdim; i++)
    for (int j = 0; j < pic->ydim; j++)
      fprintf(fp, "%d %d LN\n", i * XSTEP + XSTEP / 2 + ((j % 2) ? pic->offset : 0), j * pic->ystep + pic->ystep / 2);
  fprintf(fp, "%d setlinewidth\n1 setlinejoin\n1 setlinecap\n0 setgray\n", XSTEP / 10);
  int first = 1;
  for (long r = 0; r < n; r++) {
    if (ret[r] == 0 || idx[r] < 0) {
      if (!first) fprintf(fp, "stroke\n");
      first = 1;
      continue;
    }
    unit_position(pic, idx[r], &xp, &yp);
    if (first) fprintf(fp, "newpath\n%d %d moveto\n", xp, yp);
    else fprintf(fp, "%d %d lineto\n", xp, yp);
    first = 0;
  }
  fprintf(fp, "stroke\n");
  if (pic->ps) fprintf(fp, "showpage\n");
  return fclose(fp) != 0;
}

int main(int argc, char **argv)
{
  global_options(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *in_code_file = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *in_data_file = extract_parameter(argc, argv, "-din", OPTION);
  int plane = (int)oatoi(extract_parameter(argc, argv, "-plane", OPTION), 1);
  (void)oatoi(extract_parameter(argc, argv, "-buffer", OPTION), 0);
  struct picture pic;
  memset(&pic, 0, sizeof pic);
  pic.ps = (int)oatoi(extract_parameter(argc, argv, "-ps", OPTION), 0);
  char *funcname = extract_parameter(argc, argv, "-selfuncs", OPTION);
  if (funcname && strcasecmp(funcname, "hip") != 0 && strcasecmp(funcname, "default") != 0)
    fprintf(stderr, "functions for '%s' not found, using defaults\n", funcname);

  char *base = strdup(in_code_file), *dot = strrchr(base, '.');
  if (dot) *dot = 0;

  ifverbose(2) fprintf(stderr, "Codebook entries are read from file %s\n", in_code_file);
  struct entries *codes = open_entries(in_code_file, 0, 1), *data = NULL;
  if (!codes) { fprintf(stderr, "cant open code file '%s'\n", in_code_file); return 1; }
  if (codes->topol < TOPOL_HEXA) { printf("File %s is not a map file\n", in_code_file); return 1; }
  if (in_data_file) {
    ifverbose(2) fprintf(stderr, "Data entries are read from file %s\n", in_data_file);
    data = open_entries(in_data_file, 0, 0);             /* rows with every component masked are kept: they break the path */
    if (!data) { fprintf(stderr, "cant open data file '%s'\n", in_data_file); return 1; }
    if (data->dimension > codes->dimension) { fprintf(stderr, "Dimensions in data and codebook files are different"); return 1; }
  }
  if (plane > codes->dimension) { fprintf(stderr, "Required plane is bigger than codebook vector dimension"); return 1; }
  if (plane < 0) { fprintf(stderr, "planes: -plane %d: planes are counted from 1 (0 = all)\n", plane); return 1; }
  if (codes->masks) {
    fprintf(stderr, "planes: codebook %s has masked components (x); planes of masked codebooks are not supported\n", in_code_file);
    return 1;
  }
  if (codes->num_entries != (long)codes->xdim * codes->ydim) {
    fprintf(stderr, "planes: codebook %s has %ld entries, its %d x %d map needs %ld\n", in_code_file, codes->num_entries,
            codes->xdim, codes->ydim, (long)codes->xdim * codes->ydim);
    return 1;
  }
  if (data && data->dimension != codes->dimension) {
    fprintf(stderr, "planes: data %s has %d components, codebook %s has %d\n", in_data_file, data->dimension, in_code_file,
            codes->dimension);
    return 1;
  }

  pic.xdim = codes->xdim; pic.ydim = codes->ydim;
  pic.ystep = codes->topol == TOPOL_HEXA ? (int)(XSTEP * 0.87) : XSTEP;
  pic.offset = codes->topol == TOPOL_HEXA ? XSTEP / 2 : 0;
  pic.xsize = XSTEP * codes->xdim + pic.offset;
  pic.ysize = pic.ystep * codes->ydim;

  somhip_engine *en = NULL;
  somhip_codebook *cb = NULL;
  if (somhip_engine_create(0, &en)) { fprintf(stderr, "%s\n", somhip_last_error()); return 1; }
  if (somhip_codebook_create(en, codes->points, NULL, codes->num_entries, codes->dimension, codes->topol, codes->neigh,
                             codes->xdim, codes->ydim, 0, codes->num_entries, &cb)) {
    fprintf(stderr, "%s\n", somhip_last_error());
    return 1;
  }

  const long n = codes->num_entries;
  const int first = plane == 0 ? 0 : plane - 1, last = plane == 0 ? codes->dimension : plane;
  long slab = SLAB_BYTES / (long)(sizeof(float) * (size_t)n);
  if (slab < 1) slab = 1;
  if (slab > last - first) slab = last - first;
  float *grey = malloc(sizeof(float) * (size_t)slab * (size_t)n);
  if (!grey) { fprintf(stderr, "planes: out of memory\n"); return 1; }
  int rc = 0;
  for (int p0 = first; p0 < last && !rc; p0 += (int)slab) {
    const int count = last - p0 < slab ? last - p0 : (int)slab;
    if (somhip_planes(cb, p0, count, grey, NULL, NULL)) { fprintf(stderr, "%s\n", somhip_last_error()); return 1; }
    for (int j = 0; j < count && !rc; j++) rc = write_plane(base, &pic, codes, p0 + j, grey + (size_t)j * (size_t)n);
  }
  free(grey);

  if (data && !rc) {
    const long rows = data->num_entries;
    if (data->is_virtual && pak_materialize(data)) return 1;
    somhip_dataset *ds = NULL;
    int32_t *idx = malloc(sizeof(int32_t) * (rows + 1)), *ret = malloc(sizeof(int32_t) * (rows + 1));
    float *diff = malloc(sizeof(float) * (rows + 1));
    if (rows > 0 &&
        (somhip_dataset_create(en, data->points, rows, data->dimension, (const uint8_t *)data->masks, NULL, NULL, NULL, &ds) ||
         somhip_find_winners(cb, ds, 0, rows, 1, SOMHIP_TIE_FIRST, idx, diff, ret))) {
      fprintf(stderr, "%s\n", somhip_last_error());
      return 1;
    }
    rc = write_trajectory(base, &pic, rows, idx, ret);
    if (ds) somhip_dataset_destroy(ds);
    free(idx); free(ret); free(diff);
  }
  somhip_codebook_destroy(cb);
  close_entries(codes);
  if (data) close_entries(data);
  somhip_engine_destroy(en);
  free(base);
  return rc;
}
