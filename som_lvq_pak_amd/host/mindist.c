/* mindist -- the medians of the shortest within-class distances of a codebook (LVQ_PAK mindist.c:41-116), and with
 * -din the per-class standard deviations of a data file around the class means (deviations, lvq_rout.c:929-1004).
 * The nearest later entry of the same class of every codebook entry comes from the MI355X engine (med_distances,
 * pak_engine.c); the deviations are one pass over the data on the host. */
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "mindist - displays the medians of the shortest distances in each class (MI355X engine)\n"
    "Required:  -cin file\nOptional:  -din file  -buffer N  -v level\n";

int main(int argc, char **argv)
{
  global_options(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *in_code_file = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *in_data_file = extract_parameter(argc, argv, "-din", OPTION);
  /* -buffer only changes how the reference reads the data for the single pass of deviations: same numbers */
  (void)extract_parameter(argc, argv, "-buffer", OPTION);

  if (pak_gen_unlabelled(in_code_file) || (in_data_file && pak_gen_unlabelled(in_data_file))) {
    fprintf(stderr, "mindist: a gen: source needs labels=1 here (the classes are its labels)\n");
    exit(1);
  }
  ifverbose(2) fprintf(stderr, "Codebook entries are read from file %s\n", in_code_file);
  struct entries *codes = open_entries(in_code_file, 1, 1);
  if (!codes) { fprintf(stderr, "Can't read code file '%s'\n", in_code_file); exit(1); }
  struct entries *data = NULL;
  if (in_data_file) {
    ifverbose(2) fprintf(stderr, "Input entries are read from file %s\n", in_data_file);
    data = open_entries(in_data_file, 1, 1);
    if (!data) { fprintf(stderr, "Can't read code file '%s'\n", in_code_file); close_entries(codes); exit(1); }   /* (sic, mindist.c:74) */
    if (data->dimension != codes->dimension) {
      fprintf(stderr, "Data and codes have different dimensions\n");
      close_entries(codes); close_entries(data); exit(1);
    }
  }

  ifverbose(2) fprintf(stderr, "The medians of the shortest distances are computed\n");
  struct mindists *md = med_distances(codes);
  if (!md) exit(1);
  if (data) {
    ifverbose(2) fprintf(stderr, "The standard deviations are computed\n");
    if (deviations(data, md)) exit(1);
  }
  for (long i = 0; i < md->num_classes; i++) {               /* mindist.c:95-106 */
    fprintf(stdout, "In class %9s %3d units, min dist.: %6.3f", find_conv_to_lab((int)md->cls[i]), (int)md->noe[i], md->dists[i]);
    if (md->devs) fprintf(stdout, ", stand. dev.: %6.3f \n", md->devs[i]);
    else fprintf(stdout, "\n");
  }
  close_entries(codes);
  if (data) close_entries(data);
  free_mindists(md);
  pak_shutdown();
  return 0;
}
