/* bng -- train a codebook with batch neural gas on the MI355X engine (somhip_ng_train): every epoch ranks the units of the
 * frozen codebook by distance for every sample and replaces every unit by the mean of the data weighted by
 * exp(-rank / lambda), lambda going from -lambda down to -lambda_end over -epochs epochs.  No lattice, no labels, no
 * learning rate; the result does not depend on the order of the data beyond the order of its sums, and is the same on
 * every run.  Beyond 256 units the ranks are truncated at the 256 nearest; -dense (somhip_ng_train_dense) feeds every unit
 * of a codebook of up to 4096 rows instead, with sums formed on the fp64 MFMA.  This project's own tool: SOM_PAK and LVQ_PAK
 * have none. */
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "bng - train a codebook, batch neural gas (MI355X engine)\n"
    "Required:  -cin file  -din file  -cout file  -epochs T\n"
    "Optional:  -lambda L0 (the neighbourhood range in ranks the run starts from; default min(units, 256) / 2)\n"
    "           -lambda_end Le (... and ends at; default 0.01)\n"
    "           -ranks K (the nearest units every sample feeds, 1 .. 256; default 1 + floor(17 lambda), at most 256)\n"
    "           -dense (every unit is fed, whatever its rank: no truncation, at most 4096 units, no -ranks)\n"
    "           -v (one line per epoch to stdout: epoch, lambda, ranks and the quantization error before it)\n"
    "Any codebook is taken; its header and labels are written back as they were read.\n"
    "Files:     text (.dat/.cod), raw fp32 (a name ending in .f32; see datconv), or -din gen:k=..,dim=..,n=..,seed=..\n";

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
  char *lambda_s = extract_parameter(argc, argv, "-lambda", OPTION);
  double lambda0 = lambda_s ? atof(lambda_s) : 0.0;
  char *lambda_end_s = extract_parameter(argc, argv, "-lambda_end", OPTION);
  double lambda_end = lambda_end_s ? atof(lambda_end_s) : 0.01;
  char *ranks_s = extract_parameter(argc, argv, "-ranks", OPTION);
  long ranks = oatoi(ranks_s, 0);
  int dense = extract_parameter(argc, argv, "-dense", OPTION2) != NULL;
  if (epochs < 1) { fprintf(stderr, "bng: -epochs %ld < 1\n", epochs); exit(1); }
  if (lambda_s && !(lambda0 > 0.0)) { fprintf(stderr, "bng: -lambda %g is not a positive number\n", lambda0); exit(1); }
  if (!(lambda_end > 0.0)) { fprintf(stderr, "bng: -lambda_end %g is not a positive number\n", lambda_end); exit(1); }
  if (ranks < 0 || ranks > 256) { fprintf(stderr, "bng: -ranks %ld outside 0 .. 256\n", ranks); exit(1); }
  if (dense && ranks_s) { fprintf(stderr, "bng: -dense feeds every rank: -ranks %s cannot go with it\n", ranks_s); exit(1); }

  pak_gen_virtual_ok = 1;                                /* a gen: source is generated in HBM, never on the host */
  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (pak_masked_inputs("bng", &io, cin, din, "")) goto end;
  if (dense && io.codes->num_entries > SOMHIP_NG_DENSE_MAX) {
    fprintf(stderr, "bng: codebook %s has %ld rows, -dense takes at most %d\n", cin, (long)io.codes->num_entries, SOMHIP_NG_DENSE_MAX);
    goto end;
  }
  if (!lambda_s) lambda0 = (double)(io.codes->num_entries < 256 ? io.codes->num_entries : 256) / 2.0;
  if (lambda_end > lambda0) { fprintf(stderr, "bng: -lambda_end %g above -lambda %g\n", lambda_end, lambda0); goto end; }
  set_teach_params(&params, io.codes, io.data, NULL);
  {
    struct ng_line *line = lines ? calloc((size_t)epochs, sizeof *line) : NULL;
    if (!(dense ? ng_training_dense(&params, epochs, lambda0, lambda_end, line) : ng_training(&params, epochs, lambda0, lambda_end, ranks, line))) {
      for (long t = 0; lines && t < epochs; t++)         /* the figure as the qerror tool prints it */
        fprintf(stdout, "epoch %ld lambda %.17g ranks %d qerror %f\n", t, line[t].lambda, line[t].ranks,
                line[t].qerror / (float)io.data->num_entries);
      error = pak_save_codes(io.codes, cout);
    }
    free(line);
  }
end:
  close_entries(io.data);
  close_entries(io.codes);
  pak_shutdown();
  return error;
}
