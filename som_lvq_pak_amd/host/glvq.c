/* glvq -- train a labelled codebook with batch GLVQ on the MI355X engine (somhip_glvq_train): Sato and Yamada's
 * Generalized LVQ as full-batch gradient steps of E = mean f(mu), mu = (d+ - d-) / (d+ + d-), the rate going linearly
 * from -alpha to 0 over -epochs epochs.  The result does not depend on the order of the data beyond the order of its
 * sums, and is the same on every run.  This project's own tool: LVQ_PAK has none.
 * -buffer N takes the data through the engine N rows at a time and -gpus G divides its rows over G ranks; both leave the
 * file and the -v lines of the plain run, byte for byte (the sums' chains are continued, include/somhip_glvq_pieces.h). */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "glvq - train a labelled codebook, batch GLVQ (MI355X engine)\n"
    "Required:  -cin file  -din file  -cout file  -epochs T  -alpha A\n"
    "Optional:  -sigmoid B (the cost is 1 / (1 + exp(-B mu)); without it, mu itself)\n"
    "           -v (one line per epoch to stdout: epoch, alpha, cost and accuracy before it)\n"
    "           -buffer N (the device holds N data rows at a time; same result)\n"
    "           -gpus G (one process per GPU, the data's rows divided over them; same result; not with -buffer;\n"
    "                    SOMHIP_COMM=rccl|sockets in the environment names the ranks' transport and, as with bsom,\n"
    "                    sends even one rank through it)\n"
    "-alpha has the unit of a squared distance: about the squared distance between neighbouring classes.\n"
    "Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n";

/* what the run ends with, on the one process or on rank 0: the -v lines, then the codebook */
struct glvq_out { const char *cout; long epochs; float alpha; double *cost; int64_t *correct; };
static int save_codes(struct teach_params *teach, void *arg)
{
  struct glvq_out *o = arg;
  pak_print_epoch_costs(stdout, o->epochs, o->alpha, NULL, o->cost, o->correct, teach->data->num_entries);
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
  float alpha = (float)atof(extract_parameter(argc, argv, "-alpha", ALWAYS));
  float beta = oatof(extract_parameter(argc, argv, "-sigmoid", OPTION), 0.0f);
  if (epochs < 1) { fprintf(stderr, "glvq: -epochs %ld < 1\n", epochs); exit(1); }
  pak_rate_check("glvq", "-alpha", alpha);
  pak_rate_check("glvq", "-sigmoid", beta);
  struct pak_pieces_cli pc;
  pak_pieces_cli(argc, argv, "glvq", 1, &pc);
  if (pc.gpus_s && pc.buffer_s) { fprintf(stderr, "glvq: -gpus together with -buffer is not available (give one of the two)\n"); exit(1); }

  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (pak_masked_inputs("glvq", &io, cin, din, "")) goto end;
  if (pak_labelled_inputs("glvq", &io, cin, din)) goto end;
  set_teach_params(&params, io.codes, io.data, NULL);
  params.alpha = alpha;
  {
    double *cost = lines ? calloc((size_t)epochs, sizeof *cost) : NULL;
    int64_t *correct = lines ? calloc((size_t)epochs, sizeof *correct) : NULL;
    struct glvq_out out = {cout, epochs, alpha, cost, correct};
    if (!pc.buffer_s && (pc.gpus > 1 || getenv("SOMHIP_COMM")))  /* the ranks train, as in bsom; rank 0 prints and saves */
      error = glvq_training_multi(&params, epochs, beta, cost, correct, pc.gpus, save_codes, &out);
    else if (!(pc.buffer_s ? glvq_training_buffered(&params, epochs, pc.buffer, beta, cost, correct)
                        : glvq_training(&params, epochs, beta, cost, correct)))
      error = save_codes(&params, &out);
    free(cost);
    free(correct);
  }
end:
  close_entries(io.data);
  close_entries(io.codes);
  pak_shutdown();
  return error;
}
