/* umatrix_host_loop.c -- the U-matrix of a map on one CPU thread: the yardstick somhip_umatrix is measured against
 * (profiles/umatrix_vs_host.txt).  The project's own loop over the same arithmetic as kernels/umat.hpp: float
 * differences, double sums in component order, medians at the unit positions, scaling, then the average and the median
 * filter.  Prints its wall time and a hash of the matrix' bits, which tools/umatrix_measure.py compares with the
 * engine's.
 *
 *   gcc -O3 -ffp-contract=off -o build/umatrix_host_loop tools/umatrix_host_loop.c -lm
 *   build/umatrix_host_loop rows.f32 256 256 512 hexa        (rows.f32: xdim * ydim * dim raw floats, unit order)
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

static int mx, my, dim, ux, uy, rect;
static const float *rows;

static double pair(long a, long b)
{
  const float *pa = rows + a * dim, *pb = rows + b * dim;
  double sum = 0;
  for (int k = 0; k < dim; k++) {
    double t = pa[k] - pb[k];
    sum += t * t;
  }
  return sum;
}

struct list { int n; float v[7]; };
static void put(struct list *l, const float *u, int x, int y)
{
  if (x >= 0 && y >= 0 && x < ux && y < uy) l->v[l->n++] = u[(long)y * ux + x];
}
static int cmp_float(const void *a, const void *b)
{
  float x = *(const float *)a, y = *(const float *)b;
  return x < y ? -1 : x > y ? 1 : 0;
}

static void distances(float *u)
{
  for (int j = 0; j < my; j++)
    for (int i = 0; i < mx; i++) {
      const long k = (long)j * mx + i;
      float *below = u + (long)(2 * j + 1) * ux;
      if (i < mx - 1) u[(long)2 * j * ux + 2 * i + 1] = sqrt(pair(k, k + 1));
      if (j == my - 1) continue;
      if (rect) {
        below[2 * i] = sqrt(pair(k, k + mx));
        if (i < mx - 1) below[2 * i + 1] = (sqrt(pair(k, k + mx + 1)) / sqrt(2.0) + sqrt(pair(k + mx, k + 1)) / sqrt(2.0)) / 2;
      } else {
        below[2 * i] = sqrt(pair(k, k + mx));
        if (!(j & 1) && i > 0) below[2 * i - 1] = sqrt(pair(k, k + mx - 1));
        if ((j & 1) && i < mx - 1) below[2 * i + 1] = sqrt(pair(k, k + mx + 1));
      }
    }
}

static void unit_medians(float *u)
{
  for (int y = 0; y < uy; y += 2)
    for (int x = 0; x < ux; x += 2) {
      struct list l = {0};
      put(&l, u, x - 1, y); put(&l, u, x + 1, y);
      if (rect) { put(&l, u, x, y - 1); put(&l, u, x, y + 1); }
      else {
        const int s = (y % 4) ? 0 : -1;
        put(&l, u, x + s, y - 1); put(&l, u, x + s + 1, y - 1); put(&l, u, x + s, y + 1); put(&l, u, x + s + 1, y + 1);
      }
      qsort(l.v, l.n, sizeof(float), cmp_float);
      u[(long)y * ux + x] = (l.n & 1) ? l.v[l.n / 2] : (float)(((double)l.v[l.n / 2 - 1] + (double)l.v[l.n / 2]) / 2.0);
    }
}

/* the entries both filters read at (x, y), in the order the average adds them */
static void filter_list(struct list *l, const float *u, int x, int y, int twice_w)
{
  const int xe = ux - 1, ye = uy - 1;
  l->n = 0;
  if ((x == 0 || x == xe) && (y == 0 || y == ye)) {
    const int ix = x == 0 ? 1 : -1, iy = y == 0 ? 1 : -1;
    if (rect) {
      if (x == 0 && y == 0) { put(l, u, x + ix, y); put(l, u, x, y + iy); put(l, u, x, y); }
      else { put(l, u, x + ix, y); put(l, u, x, y); put(l, u, x, y + iy); }
    } else if (x == 0 && y == 0) { put(l, u, 1, 0); put(l, u, 0, 0); put(l, u, 0, 1); }
    else if (y == 0) { put(l, u, x, 0); put(l, u, x, 1); put(l, u, x - 1, 0); put(l, u, x - 1, 1); }
    else if (x == 0) { put(l, u, 0, y); put(l, u, 1, y); put(l, u, 0, y - 1); }
    else { put(l, u, x, y); put(l, u, x, y - 1); put(l, u, x - 1, y); }
    return;
  }
  if (rect) {
    put(l, u, x, y - 1); put(l, u, x - 1, y);
    if (twice_w && x == xe) put(l, u, x - 1, y);
    put(l, u, x, y); put(l, u, x + 1, y); put(l, u, x, y + 1);
    return;
  }
  const int r = y % 4, up = (r == 1 || r == 2) ? 0 : -1, down = (r == 0 || r == 1) ? -1 : 0;
  put(l, u, x + up, y - 1); put(l, u, x + up + 1, y - 1);
  put(l, u, x - 1, y); put(l, u, x, y); put(l, u, x + 1, y);
  put(l, u, x + down, y + 1); put(l, u, x + down + 1, y + 1);
}

int main(int argc, char **argv)
{
  if (argc != 6) { fprintf(stderr, "usage: %s rows.f32 xdim ydim dim hexa|rect\n", argv[0]); return 1; }
  mx = atoi(argv[2]); my = atoi(argv[3]); dim = atoi(argv[4]); rect = strcmp(argv[5], "rect") == 0;
  if (mx < 2 || my < 2 || dim < 1) { fprintf(stderr, "bad shape\n"); return 1; }
  ux = 2 * mx - 1; uy = 2 * my - 1;
  const size_t n = (size_t)mx * my * dim, count = (size_t)ux * uy;
  float *r = malloc(sizeof(float) * n), *u = calloc(count, sizeof(float)), *v = malloc(sizeof(float) * count);
  FILE *fp = fopen(argv[1], "rb");
  if (!fp || fread(r, sizeof(float), n, fp) != n) { fprintf(stderr, "can't read %zu floats from %s\n", n, argv[1]); return 1; }
  fclose(fp);
  rows = r;
  struct timespec t0, t1, t2;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  distances(u);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  unit_medians(u);
  double lo = u[0], hi = u[0];
  for (size_t t = 0; t < count; t++) { if (u[t] > hi) hi = u[t]; if (u[t] < lo) lo = u[t]; }
  for (size_t t = 0; t < count; t++) u[t] = 1.0 - (u[t] - lo) / (hi - lo);
  struct list l;
  for (int y = 0; y < uy; y++)
    for (int x = 0; x < ux; x++) {
      filter_list(&l, u, x, y, 0);
      float sum = l.v[0];
      for (int a = 1; a < l.n; a++) sum = sum + l.v[a];
      v[(long)y * ux + x] = rect ? (float)(sum / (double)l.n) : sum / (float)l.n;
    }
  for (int y = 0; y < uy; y++)
    for (int x = 0; x < ux; x++) {
      filter_list(&l, v, x, y, 1);
      qsort(l.v, l.n, sizeof(float), cmp_float);
      u[(long)y * ux + x] = l.v[l.n / 2];
    }
  clock_gettime(CLOCK_MONOTONIC, &t2);
  uint64_t h = 1469598103934665603ull;
  for (size_t t = 0; t < count; t++) { uint32_t b; memcpy(&b, &u[t], 4); h = (h ^ b) * 1099511628211ull; }
  printf("host umatrix: %d x %d x %d %s, average + median: distances %.3f s, all %.3f s on one thread; min %.9g max %.9g; hash %016llx\n",
         mx, my, dim, argv[5], (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec),
         (t2.tv_sec - t0.tv_sec) + 1e-9 * (t2.tv_nsec - t0.tv_nsec), lo, hi, (unsigned long long)h);
  return 0;
}
