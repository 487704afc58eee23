/* med_distances_host_loop.c -- the host loop that `balance` carried before the within-class nearest-neighbour search
 * moved to the engine (somhip_class_nearest_later): the reference's med_distances (lvq_rout.c:384-491) with
 * vector_dist_euc (lvq_pak.c:291-316) on one CPU thread.  Kept as the yardstick the kernel is measured against
 * (profiles/class_nearest_vs_host.txt): prints the class table `stddev` prints for the medians, and its wall time.
 *
 *   gcc -O3 -ffp-contract=off -fopenmp -Iinclude -Isom_lvq_pak_amd/host -o build/med_distances_host_loop \
 *       tools/med_distances_host_loop.c som_lvq_pak_amd/host/pak_io.c -lm
 *   build/med_distances_host_loop gen:k=16,dim=128,n=65536,seed=1,labels=1
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "pak.h"

/* vector_dist_euc, lvq_pak.c:291-316 */
static float dist_euc(const struct data_entry *a, const struct data_entry *b, int dim)
{
  float diff, difference = 0.0;
  int masked = 0;
  for (int i = 0; i < dim; i++) {
    if ((a->mask && a->mask[i]) || (b->mask && b->mask[i])) masked++;
    else { diff = a->points[i] - b->points[i]; difference += diff * diff; }
  }
  if (masked == dim) return -1;
  return sqrt(difference);
}

static int cmp_float(const void *a, const void *b)
{
  float x = *(const float *)a, y = *(const float *)b;
  return x < y ? -1 : x > y ? 1 : 0;
}

struct host_mindists { long num_classes; long *cls; long *noe; float *dists; };

/* med_distances, lvq_rout.c:373-491: per class (most frequent first), the median over its entries
 * of the distance to the nearest LATER entry of the same class */
static struct host_mindists *host_med_distances(struct entries *codes)
{
  struct host_mindists *md = calloc(1, sizeof *md);
  struct hitlist *classes = new_hitlist();
  int dim = codes->dimension;
  for (long r = 0; r < codes->num_entries; r++) add_hit(classes, get_entry_label(&codes->rows[r]));
  long nol = classes->entries;
  md->num_classes = nol;
  md->cls = calloc(nol + 1, sizeof(long)); md->noe = calloc(nol + 1, sizeof(long)); md->dists = calloc(nol + 1, sizeof(float));
  long mnoe = nol ? classes->freq[0] : 0;
  float *meds = malloc(sizeof(float) * (mnoe + 1));
  for (long i = 0; i < nol; i++) {
    md->cls[i] = classes->label[i];
    md->noe[i] = classes->freq[i];
    long not = 0;
    for (long r = 0; r < codes->num_entries; r++) {
      if (get_entry_label(&codes->rows[r]) != md->cls[i]) continue;
      float dissf = FLT_MAX;
      int fou = 0;
      for (long s = r + 1; s < codes->num_entries; s++)
        if (get_entry_label(&codes->rows[s]) == md->cls[i]) {
          fou = 1;
          float dist = dist_euc(&codes->rows[s], &codes->rows[r], dim);
          if (dist < dissf) dissf = dist;
        }
      if (fou) meds[not++] = dissf;
    }
    if (not > 0) { qsort(meds, not, sizeof(float), cmp_float); md->dists[i] = meds[not / 2]; }
  }
  free(meds); free_hitlist(classes);
  return md;
}

int main(int argc, char **argv)
{
  if (argc != 2) { fprintf(stderr, "usage: %s file|gen:spec\n", argv[0]); return 1; }
  struct entries *data = open_entries(argv[1], 1, 1);
  if (!data) return 1;
  struct timespec t0, t1;
  clock_gettime(CLOCK_MONOTONIC, &t0);
  struct host_mindists *md = host_med_distances(data);
  clock_gettime(CLOCK_MONOTONIC, &t1);
  for (long i = 0; i < md->num_classes; i++)
    fprintf(stdout, "In class %9s %3d units, med dist.: %6.3f\n", find_conv_to_lab((int)md->cls[i]), (int)md->noe[i], md->dists[i]);
  fprintf(stdout, "host med_distances: %ld rows x %d, %.3f s on one thread\n", data->num_entries, data->dimension,
          (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
  return 0;
}
