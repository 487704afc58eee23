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

/* 1 after a message when a row of e has no label */
static int unlabelled(struct entries *e, const char *what, const char *name)
{
  for (long r = 0; r < e->num_entries; r++)
    if (get_entry_label(&e->rows[r]) == LABEL_EMPTY) {
      fprintf(stderr, "glvq: %s %s has no labels on row %ld\n", what, name, r);
      return 1;
    }
  return 0;
}

/* what the run ends with, on the one process or on rank 0: the -v lines, then the codebook */
struct glvq_out { const char *cout; long epochs; float alpha; double *cost; int64_t *correct; };
static int save_codes(struct teach_params *teach, void *arg)
{
  struct glvq_out *o = arg;
  for (long t = 0; o->cost && t < o->epochs; t++) {
    const float a = o->alpha * (float)(o->epochs - t) / (float)o->epochs;   /* the engine's alpha_t */
    fprintf(stdout, "epoch %ld alpha %.9g cost %.17g accuracy %.2f %%\n", t, (double)a, o->cost[t],
            100.0 * (double)o->correct[t] / (double)teach->data->num_entries);
  }
  ifverbose(2) fprintf(stderr, "Codebook entries are saved to file %s\n", o->cout);
  return save_entries(teach->codes, (char *)o->cout) ? 1 : 0;
}

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
  float alpha = (float)atof(extract_parameter(argc, argv, "-alpha", ALWAYS));
  float beta = oatof(extract_parameter(argc, argv, "-sigmoid", OPTION), 0.0f);
  if (epochs < 1) { fprintf(stderr, "glvq: -epochs %ld < 1\n", epochs); exit(1); }
  if (!(alpha >= 0.0f)) { fprintf(stderr, "glvq: -alpha %g is negative or not a number\n", (double)alpha); exit(1); }
  if (!(beta >= 0.0f)) { fprintf(stderr, "glvq: -sigmoid %g is negative or not a number\n", (double)beta); exit(1); }
  char *buffer_s = extract_parameter(argc, argv, "-buffer", OPTION), *gpus_s = extract_parameter(argc, argv, "-gpus", OPTION);
  long buffer = oatoi(buffer_s, 0);
  int gpus = (int)oatoi(gpus_s, 1);
  if (buffer_s && buffer < 1) { fprintf(stderr, "glvq: -buffer %ld < 1\n", buffer); exit(1); }
  if (gpus < 1 || gpus > 64) { fprintf(stderr, "glvq: -gpus %d outside 1 .. 64\n", gpus); exit(1); }
  if (gpus_s && buffer_s) { fprintf(stderr, "glvq: -gpus together with -buffer is not available (give one of the two)\n"); exit(1); }

  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (io.codes->masks) { fprintf(stderr, "glvq: codebook %s has masked components (x): not supported\n", cin); goto end; }
  if (io.data->masks) { fprintf(stderr, "glvq: data %s has masked components (x): not supported\n", din); goto end; }
  if (unlabelled(io.codes, "codebook", cin) || unlabelled(io.data, "data", din)) goto end;
  {                                                      /* the labels of the two files, before an engine is asked for */
    const long noc = io.codes->num_entries;
    int one = 1;
    for (long r = 1; r < noc; r++) one &= get_entry_label(&io.codes->rows[r]) == get_entry_label(&io.codes->rows[0]);
    if (one) { fprintf(stderr, "glvq: every row of codebook %s carries one label (no other class to be wrong with)\n", cin); goto end; }
    for (long s = 0; s < io.data->num_entries; s++) {
      const int l = get_entry_label(&io.data->rows[s]);
      long r = 0;
      while (r < noc && get_entry_label(&io.codes->rows[r]) != l) r++;
      if (r == noc) { fprintf(stderr, "glvq: data row %ld carries label %s, which no codebook row carries\n", s, find_conv_to_lab(l)); goto end; }
    }
  }
  set_teach_params(&params, io.codes, io.data, NULL);
  params.alpha = alpha;
  {
    double *cost = lines ? calloc((size_t)epochs, sizeof *cost) : NULL;
    int64_t *correct = lines ? calloc((size_t)epochs, sizeof *correct) : NULL;
    struct glvq_out out = {cout, epochs, alpha, cost, correct};
    if (!buffer_s && (gpus > 1 || getenv("SOMHIP_COMM")))  /* the ranks train, as in bsom; rank 0 prints and saves */
      error = glvq_training_multi(&params, epochs, beta, cost, correct, gpus, save_codes, &out);
    else if (!(buffer_s ? glvq_training_buffered(&params, epochs, buffer, beta, cost, correct)
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
