/* bsom -- teach a self-organizing map with Kohonen's batch map on the MI355X engine (somhip_som_batchmap): every epoch
 * finds the winners of the whole data set against the frozen map and replaces every model vector by the
 * neighbourhood-weighted mean of the data, the radius going from -radius down to 1 over -epochs epochs.  No learning
 * rate; the result does not depend on the order of the data.  This project's own tool: SOM_PAK has none.
 * -buffer N takes the data through the engine N rows at a time and -gpus G divides its rows over G ranks; both leave the
 * file and the -v lines of the plain run, byte for byte (the sums' chains are continued, include/somhip.h).
 * -missing takes data whose samples leave components out (x): a sample is matched over the components it has and a
 * component of a model vector becomes the weighted mean of the samples that know it
 * (include/somhip_batchmap_missing.h); on data without x it writes the plain run's bytes. */
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "bsom - teach self-organizing map, batch map (MI355X engine)\n"
    "Required:  -cin file  -din file  -cout file  -epochs T  -radius R\n"
    "Optional:  -v (one line per epoch to stdout: epoch, radius, quantization error before it)\n"
    "           -buffer N (the device holds N data rows at a time; same result)\n"
    "           -gpus G (one process per GPU, the data's rows divided over them; same result; not with -buffer;\n"
    "                    SOMHIP_COMM=rccl|sockets in the environment names the ranks' transport and, as with vsom,\n"
    "                    sends even one rank through it)\n"
    "           -missing (take data with missing components, x: a sample is matched over the components it has, a\n"
    "                     component of a model vector becomes the mean of the samples that know it; data without x\n"
    "                     give the same map as without the option; works with -buffer, not with -gpus)\n"
    "Topology and neighbourhood come from the codebook's header.\n"
    "Files:     text (.dat/.cod), raw fp32 (a name ending in .f32; see datconv), or -din gen:k=..,dim=..,n=..,seed=..\n";

/* what the run ends with, on the one process or on rank 0: the -v lines, then the codebook */
struct bsom_out { const char *cout; long epochs; float radius; float *qerror; };
static int save_codes(struct teach_params *teach, void *arg)
{
  struct bsom_out *o = arg;
  for (long t = 0; o->qerror && t < o->epochs; t++)
    fprintf(stdout, "epoch %ld radius %.9g qerror %.9g\n", t, (double)pak_linear_radius(o->radius, o->epochs, t), (double)o->qerror[t]);
  return pak_save_codes(teach->codes, o->cout);
}

int main(int argc, char **argv)
{
  struct teach_params params;
  struct pak_inputs io = {NULL, NULL};
  int error = 1;

  memset(&params, 0, sizeof params);
  int lines = pak_batch_verbose(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *din = extract_parameter(argc, argv, "-din", ALWAYS), *cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *cout = extract_parameter(argc, argv, "-cout", ALWAYS);
  long epochs = oatoi(extract_parameter(argc, argv, "-epochs", ALWAYS), 0);
  float radius = (float)atof(extract_parameter(argc, argv, "-radius", ALWAYS));
  if (epochs < 1) { fprintf(stderr, "bsom: -epochs %ld < 1\n", epochs); exit(1); }
  if (!(radius >= 1.0f)) { fprintf(stderr, "bsom: -radius %g < 1\n", (double)radius); exit(1); }
  struct pak_pieces_cli pc;
  pak_pieces_cli(argc, argv, "bsom", 0, &pc);
  int missing = extract_parameter(argc, argv, "-missing", OPTION2) != NULL;
  if (missing && pc.gpus_s) { fprintf(stderr, "bsom: -missing together with -gpus is not available (the ranks train without masks)\n"); exit(1); }
  if (pc.gpus_s && pc.buffer_s) { fprintf(stderr, "bsom: -gpus together with -buffer is not available (give one of the two)\n"); exit(1); }

  pak_gen_virtual_ok = 1;                                /* a gen: source is generated in HBM, never on the host */
  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 1, &io)) goto end;
  if (pak_masked_inputs("bsom", &io, cin, din, missing ? NULL : " without -missing")) goto end;
  set_teach_params(&params, io.codes, io.data, NULL);
  params.radius = radius;
  float *qerror = lines ? calloc((size_t)epochs, sizeof *qerror) : NULL;
  struct bsom_out out = {cout, epochs, radius, qerror};
  if (missing) {
    if (!som_batchmap_missing_training(&params, epochs, pc.buffer, qerror)) error = save_codes(&params, &out);
  } else if (!pc.buffer_s && (pc.gpus > 1 || getenv("SOMHIP_COMM")))  /* the ranks train, as in vsom; rank 0 prints and saves */
    error = som_batchmap_training_multi(&params, epochs, qerror, pc.gpus, save_codes, &out);
  else if (!som_batchmap_training(&params, epochs, pc.buffer, qerror))
    error = save_codes(&params, &out);
  free(qerror);
end:
  close_entries(io.data);
  close_entries(io.codes);
  pak_shutdown();
  return error;
}
