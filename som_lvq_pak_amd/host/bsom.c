/* bsom -- teach a self-organizing map with Kohonen's batch map on the MI355X engine (somhip_som_batchmap): every epoch
 * finds the winners of the whole data set against the frozen map and replaces every model vector by the
 * neighbourhood-weighted mean of the data, the radius going from -radius down to 1 over -epochs epochs.  No learning
 * rate; the result does not depend on the order of the data.  This project's own tool: SOM_PAK has none. */
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "bsom - teach self-organizing map, batch map (MI355X engine)\n"
    "Required:  -cin file  -din file  -cout file  -epochs T  -radius R\n"
    "Optional:  -v (one line per epoch to stdout: epoch, radius, quantization error before it)\n"
    "Topology and neighbourhood come from the codebook's header.\n"
    "Files:     text (.dat/.cod), raw fp32 (a name ending in .f32; see datconv), or -din gen:k=..,dim=..,n=..,seed=..\n";

int main(int argc, char **argv)
{
  struct teach_params params;
  struct pak_inputs io = {NULL, NULL};
  int error = 1;

  memset(&params, 0, sizeof params);
  int lines = extract_parameter(argc, argv, "-v", OPTION2) != NULL;
  global_options(argc, argv);
  char *level = extract_parameter(argc, argv, "-v", OPTION);
  if (lines && (!level || level[0] == '-')) verbose_level = 1;   /* a bare -v: the next argument is no level */
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *din = extract_parameter(argc, argv, "-din", ALWAYS), *cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *cout = extract_parameter(argc, argv, "-cout", ALWAYS);
  long epochs = oatoi(extract_parameter(argc, argv, "-epochs", ALWAYS), 0);
  float radius = (float)atof(extract_parameter(argc, argv, "-radius", ALWAYS));
  if (epochs < 1) { fprintf(stderr, "bsom: -epochs %ld < 1\n", epochs); exit(1); }
  if (!(radius >= 1.0f)) { fprintf(stderr, "bsom: -radius %g < 1\n", (double)radius); exit(1); }

  pak_gen_virtual_ok = 1;                                /* a gen: source is generated in HBM, never on the host */
  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 1, &io)) goto end;
  if (io.codes->masks) { fprintf(stderr, "bsom: codebook %s has masked components (x): not supported\n", cin); goto end; }
  if (io.data->masks) { fprintf(stderr, "bsom: data %s has masked components (x): not supported\n", din); goto end; }
  set_teach_params(&params, io.codes, io.data, NULL);
  params.radius = radius;
  float *qerror = lines ? calloc((size_t)epochs, sizeof *qerror) : NULL;
  if (!som_batchmap_training(&params, epochs, qerror)) {
    for (long t = 0; qerror && t < epochs; t++) {
      const float r = 1.0f + (radius - 1.0f) * (float)(epochs - t) / (float)epochs;   /* the engine's r_t */
      fprintf(stdout, "epoch %ld radius %.9g qerror %.9g\n", t, (double)r, (double)qerror[t]);
    }
    ifverbose(2) fprintf(stderr, "Codebook entries are saved to file %s\n", cout);
    error = save_entries(io.codes, cout) ? 1 : 0;
  }
  free(qerror);
end:
  close_entries(io.data);
  close_entries(io.codes);
  pak_shutdown();
  return error;
}
