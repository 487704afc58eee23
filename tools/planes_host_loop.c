/* planes_host_loop.c -- the grey-scaled component planes of a codebook on one CPU thread: the yardstick somhip_planes is
 * measured against (profiles/planes_vs_host.txt).  The project's own loop over the same arithmetic as kernels/planes.hpp,
 * over row-major rows as somhip_codebook_download returns them: per component the smallest and the largest value, then
 * (float)(0.05 + 0.9 * (double)(p - lo) / (double)(hi - lo)) with both differences taken in float.  Prints its wall time
 * and writes the planes, plane-major, for tools/planes_measure.py to compare with the engine's.
 *
 *   gcc -O3 -ffp-contract=off -o build/planes_host_loop tools/planes_host_loop.c
 *   build/planes_host_loop rows.f32 65536 512 grey.f32        (rows.f32: n * dim raw floats, row order)
 */
#include <float.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

static double now(void)
{
  struct timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

int main(int argc, char **argv)
{
  if (argc != 5) { fprintf(stderr, "usage: planes_host_loop rows.f32 n dim grey.f32\n"); return 2; }
  const long n = atol(argv[2]);
  const int dim = atoi(argv[3]);
  float *rows = malloc(sizeof(float) * n * dim), *grey = malloc(sizeof(float) * n * dim);
  float *lo = malloc(sizeof(float) * dim), *hi = malloc(sizeof(float) * dim);
  FILE *f = fopen(argv[1], "rb");
  if (!f || !rows || !grey || fread(rows, sizeof(float), (size_t)n * dim, f) != (size_t)n * dim) { fprintf(stderr, "can't read %s\n", argv[1]); return 1; }
  fclose(f);
  const double t0 = now();
  for (int c = 0; c < dim; c++) { lo[c] = FLT_MAX; hi[c] = -FLT_MAX; }
  for (long k = 0; k < n; k++)                            /* one pass over the rows in memory order */
    for (int c = 0; c < dim; c++) {
      const float p = rows[k * dim + c];
      if (hi[c] < p) hi[c] = p;
      if (lo[c] > p) lo[c] = p;
    }
  const double t1 = now();
  for (long k = 0; k < n; k++)                            /* rows in memory order, planes written with stride n */
    for (int c = 0; c < dim; c++) {
      const float range = hi[c] - lo[c];
      float cv = 0.5f;
      if (range != 0.0f) {
        const float num = rows[k * dim + c] - lo[c];
        cv = (float)(0.05 + 0.9 * (double)num / (double)range);
      }
      grey[(long)c * n + k] = cv;
    }
  const double t2 = now();
  printf("host planes: %ld x %d: min and max %.3f s, grey levels %.3f s, all %.3f s on one thread\n", n, dim, t1 - t0, t2 - t1, t2 - t0);
  f = fopen(argv[4], "wb");
  if (!f || fwrite(grey, sizeof(float), (size_t)n * dim, f) != (size_t)n * dim) { fprintf(stderr, "can't write %s\n", argv[4]); return 1; }
  fclose(f);
  return 0;
}
