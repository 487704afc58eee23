/* somqual -- quality of a trained map on a data set: the quantization error (the qerror tool's own line), the
 * topographic error (the share of samples whose best and second-best matching units are not neighbours on the lattice)
 * and, per unit, how many samples it wins and their mean distance; with -conn, per ordered pair (best unit, second-best
 * unit) the number of samples that have it; with -distortion R, the map's distortion (its energy) at radius R.  Everything
 * is formed on the MI355X engine (somhip_map_quality, somhip_map_connectivity, somhip_distortion_*); the host prints. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "somqual - quantization error, topographic error and per-unit statistics of a map (MI355X engine)\n"
    "Required:  -cin file  -din file (.dat, raw fp32 or gen:)\n"
    "Optional:  -uout file (one line per unit: x y hits mean)  -buffer N (data rows per engine call)\n"
    "           -conn file (one line per pair of best and second-best unit: x1 y1 x2 y2 count lattice_sq)\n"
    "           -distortion R (the map's energy at radius R >= 0 with its own neighbourhood, one more line; a fifth\n"
    "                          field, the unit's share of it, on every line of -uout)\n"
    "           -selfuncs hip  -v level\n";

/* the squared lattice distance of units (bx, by) and (tx, ty), formed as the engine's lattice_sq forms it: floats, with the
 * half step of an odd row distance and the 0.75 dy^2 of a hexagonal lattice taken in double */
static float lattice_sq(int topol, int bx, int by, int tx, int ty)
{
  float dx = (float)(bx - tx), dy = (float)(by - ty);
  if (topol == TOPOL_RECT) {
    float r = dx * dx, r2 = dy * dy;
    return r + r2;
  }
  if ((by - ty) % 2 != 0) dx = (by % 2 == 0) ? (float)((double)dx - 0.5) : (float)((double)dx + 0.5);
  float r = dx * dx;
  double t = 0.75 * (double)dy;
  t = t * (double)dy;
  return (float)((double)r + t);
}

int main(int argc, char **argv)
{
  struct teach_params teach;
  struct pak_inputs io;
  struct map_quality q;
  memset(&teach, 0, sizeof teach);
  global_options(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *din = extract_parameter(argc, argv, "-din", ALWAYS), *cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *uout = extract_parameter(argc, argv, "-uout", OPTION);
  char *conn = extract_parameter(argc, argv, "-conn", OPTION);
  char *funcname = extract_parameter(argc, argv, "-selfuncs", OPTION);
  long buffer = oatoi(extract_parameter(argc, argv, "-buffer", OPTION), 0);
  float dradius = -1.0f;                                   /* < 0: no -distortion */
  if (extract_parameter(argc, argv, "-distortion", OPTION2)) {
    char *s = extract_parameter(argc, argv, "-distortion", OPTION), *end = s;
    const double v = s ? strtod(s, &end) : 0.0;
    if (!s || end == s || *end || !(v >= 0.0)) {
      fprintf(stderr, "somqual: -distortion needs a radius >= 0%s%s\n", s ? ", not " : "", s ? s : "");
      exit(1);
    }
    dradius = (float)v;
  }

  pak_gen_virtual_ok = 1;                                /* a gen: source is generated in HBM, never on the host */
  if (pak_open_inputs(din, 0, "Can't open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 2, &io)) exit(1);
  if (io.codes->masks) {
    fprintf(stderr, "somqual: codebook %s has masked components (x); the quality of masked codebooks is not supported\n", cin);
    exit(1);
  }
  set_teach_params(&teach, io.codes, io.data, funcname);
  if (find_map_quality(&teach, buffer, conn != NULL, dradius, &q)) exit(1);
  long nod = io.data->num_entries, noc = io.codes->num_entries, dead = 0;
  ifverbose(1)
    fprintf(stdout, "Quantization error of %s with map %s is %f per sample (%ld samples)\n", din, cin, q.qerror / (float)nod, nod);
  else
    fprintf(stdout, "%f\n", q.qerror / (float)nod);
  if (q.topo_defined > 0)
    fprintf(stdout, "Topographic error is %f (%ld of %ld samples)\n", (double)q.topo_errors / (double)q.topo_defined,
            q.topo_errors, q.topo_defined);
  else
    fprintf(stdout, "Topographic error is undefined (0 of 0 samples)\n");
  for (long u = 0; u < noc; u++) dead += q.hits[u] == 0;
  fprintf(stdout, "%ld of %ld units were hit by no sample\n", dead, noc);
  int rc = 0;
  if (uout) {
    FILE *fp = fopen(uout, "w");
    if (!fp) { fprintf(stderr, "somqual: can't write %s\n", uout); rc = 1; }
    else {
      for (long u = 0; u < noc; u++) {
        fprintf(fp, "%ld %ld %lu ", u % io.codes->xdim, u / io.codes->xdim, (unsigned long)q.hits[u]);
        if (q.hits[u]) fprintf(fp, "%f", q.qsum[u] / (double)q.hits[u]);
        else fprintf(fp, "0");
        if (q.unit_energy) fprintf(fp, " %.9g", q.unit_energy[u]);
        fputc('\n', fp);
      }
      if (fclose(fp)) { fprintf(stderr, "somqual: can't write %s\n", uout); rc = 1; }
    }
  }
  if (conn) {
    const int xdim = io.codes->xdim, topol = io.codes->topol;
    long apart = 0;
    FILE *fp = fopen(conn, "w");
    if (!fp) { fprintf(stderr, "somqual: can't write %s\n", conn); rc = 1; }
    for (long p = 0; p < q.n_pairs; p++) {
      const int x1 = (int)(q.b1[p] % xdim), y1 = (int)(q.b1[p] / xdim), x2 = (int)(q.b2[p] % xdim), y2 = (int)(q.b2[p] / xdim);
      const float lsq = lattice_sq(topol, x1, y1, x2, y2);
      apart += lsq > 1.0f;
      if (fp) fprintf(fp, "%d %d %d %d %llu %g\n", x1, y1, x2, y2, (unsigned long long)q.pair_count[p], (double)lsq);
    }
    fprintf(stdout, "Connected pairs (best unit, second-best unit): %ld, of which %ld are not neighbours on the lattice\n", q.n_pairs, apart);
    if (fp && fclose(fp)) { fprintf(stderr, "somqual: can't write %s\n", conn); rc = 1; }
  }
  if (q.unit_energy) {
    const double ns = (double)q.distortion_samples;
    fprintf(stdout, "Distortion at radius %g (%s neighbourhood) is %.9g per sample (%llu samples), resolved to %.3g\n", (double)dradius,
            io.codes->neigh == NEIGH_GAUSSIAN ? "gaussian" : "bubble", q.energy / ns, q.distortion_samples,
            ldexp(q.scale, -52) / ns);
  }
  free_map_quality(&q);
  close_entries(io.data); close_entries(io.codes);
  pak_shutdown();
  return rc;
}
