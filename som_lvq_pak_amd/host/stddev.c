/* stddev -- per class of a data file, the median of the shortest within-class distances and the standard deviation
 * around the class mean (LVQ_PAK stddev.c:40-88).  The nearest later entry of the same class of every data entry -- a
 * self-join of sum n_c^2 dim / 2 distance terms, hours on one core for a large file -- comes from the MI355X engine
 * (med_distances, pak_engine.c); the deviations are one pass over the data on the host. */
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "stddev - displays the medians of the shortest distances and the deviations in each class (MI355X engine)\n"
    "Required:  -din file\nOptional:  -v level\n";

int main(int argc, char **argv)
{
  global_options(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *in_data_file = extract_parameter(argc, argv, "-din", ALWAYS);
  /* The reference's med_distances walks the list with two nested cursors; over a buffered list (set_buffer, stddev.c:63)
   * the inner one ends at the buffer's edge without loading the next, and every class prints `med dist.:  0.000`. */
  if (oatoi(extract_parameter(argc, argv, "-buffer", OPTION), 0) > 0) {
    fprintf(stderr, "stddev: -buffer is not supported: the nearest-neighbour search needs the whole file at once\n");
    exit(1);
  }
  if (pak_gen_unlabelled(in_data_file)) {
    fprintf(stderr, "stddev: a gen: source needs labels=1 here (the classes are its labels)\n");
    exit(1);
  }

  ifverbose(2) fprintf(stderr, "Input entries are read from file %s\n", in_data_file);
  struct entries *data = open_entries(in_data_file, 1, 1);
  if (!data) { fprintf(stderr, "Can't read data file '%s'\n", in_data_file); exit(1); }

  struct mindists *md = med_distances(data);
  if (!md) exit(1);
  ifverbose(2) fprintf(stderr, "The standard deviations are computed\n");
  if (deviations(data, md)) exit(1);
  for (long i = 0; i < md->num_classes; i++) {               /* stddev.c:74-80 */
    fprintf(stdout, "In class %9s %3d units, med dist.: %6.3f", find_conv_to_lab((int)md->cls[i]), (int)md->noe[i], md->dists[i]);
    fprintf(stdout, ", stand. dev.: %6.3f \n", md->devs[i]);
  }
  close_entries(data);
  free_mindists(md);
  pak_shutdown();
  return 0;
}
