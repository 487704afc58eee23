/* rslvq -- train a labelled codebook with batch Robust Soft LVQ on the MI355X engine (somhip_rslvq_train): Seo and
 * Obermayer's RSLVQ as full-batch gradient steps of E = mean -log P(label | x) under a Gaussian mixture whose centres are
 * the codebook's rows, the rate going linearly from -alpha to 0 over -epochs epochs.  Every sample moves every row in
 * proportion to a posterior; the result does not depend on the order of the data beyond the order of its sums, and is
 * the same on every run.  This project's own tool: LVQ_PAK has none. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "rslvq - train a labelled codebook, batch Robust Soft LVQ (MI355X engine)\n"
    "Required:  -cin file  -din file  -epochs T  -sigma2 S  (and -cout file  -alpha A  where T > 0)\n"
    "Optional:  -pout file (one line per data row: its label and P(label | x) under the codebook the tool ends with)\n"
    "           -v (one line per epoch to stdout: epoch, alpha, cost and accuracy before it)\n"
    "-epochs 0 trains nothing and writes no codebook: it prints the cost and accuracy of -cin.\n"
    "-sigma2 is the squared width of the mixture's components; -alpha has the unit of a squared distance.\n"
    "Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n";

/* 1 after a message when a row of e has no label */
static int unlabelled(struct entries *e, const char *what, const char *name)
{
  for (long r = 0; r < e->num_entries; r++)
    if (get_entry_label(&e->rows[r]) == LABEL_EMPTY) {
      fprintf(stderr, "rslvq: %s %s has no labels on row %ld\n", what, name, r);
      return 1;
    }
  return 0;
}

/* "%.9g" is glvq's format of a rate; a probability gets the same digits */
static int write_pown(const char *name, struct entries *data, const double *pown)
{
  FILE *fp = fopen(name, "w");
  if (!fp) { fprintf(stderr, "rslvq: can't open file '%s' for writing\n", name); return 1; }
  for (long s = 0; s < data->num_entries; s++)
    fprintf(fp, "%s %.9g\n", find_conv_to_lab(get_entry_label(&data->rows[s])), pown[s]);
  return fclose(fp) ? 1 : 0;
}

int main(int argc, char **argv)
{
  struct teach_params params;
  struct pak_inputs io = {NULL, NULL};
  double *pown = NULL;
  int error = 1;

  memset(&params, 0, sizeof params);
  int lines = extract_parameter(argc, argv, "-v", OPTION2) != NULL;
  global_options(argc, argv);
  char *level = extract_parameter(argc, argv, "-v", OPTION);
  if (lines && (!level || level[0] == '-')) verbose_level = 1;   /* a bare -v: the next argument is no level */
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *din = extract_parameter(argc, argv, "-din", ALWAYS), *cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *pout = extract_parameter(argc, argv, "-pout", OPTION);
  long epochs = oatoi(extract_parameter(argc, argv, "-epochs", ALWAYS), 0);
  char *cout = extract_parameter(argc, argv, "-cout", epochs > 0 ? ALWAYS : OPTION);
  float alpha = oatof(extract_parameter(argc, argv, "-alpha", epochs > 0 ? ALWAYS : OPTION), 0.0f);
  float sigma2 = (float)atof(extract_parameter(argc, argv, "-sigma2", ALWAYS));
  if (epochs < 0) { fprintf(stderr, "rslvq: -epochs %ld < 0\n", epochs); exit(1); }
  if (!(alpha >= 0.0f)) { fprintf(stderr, "rslvq: -alpha %g is negative or not a number\n", (double)alpha); exit(1); }
  if (!(sigma2 > 0.0f) || isinf(sigma2)) { fprintf(stderr, "rslvq: -sigma2 %g is not a finite number above 0\n", (double)sigma2); exit(1); }

  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (io.codes->masks) { fprintf(stderr, "rslvq: codebook %s has masked components (x): not supported\n", cin); goto end; }
  if (io.data->masks) { fprintf(stderr, "rslvq: data %s has masked components (x): not supported\n", din); goto end; }
  if (unlabelled(io.codes, "codebook", cin) || unlabelled(io.data, "data", din)) goto end;
  {                                                      /* the labels of the two files, before an engine is asked for */
    const long noc = io.codes->num_entries;
    int one = 1;
    for (long r = 1; r < noc; r++) one &= get_entry_label(&io.codes->rows[r]) == get_entry_label(&io.codes->rows[0]);
    if (one) { fprintf(stderr, "rslvq: every row of codebook %s carries one label (no other class to be wrong with)\n", cin); goto end; }
    for (long s = 0; s < io.data->num_entries; s++) {
      const int l = get_entry_label(&io.data->rows[s]);
      long r = 0;
      while (r < noc && get_entry_label(&io.codes->rows[r]) != l) r++;
      if (r == noc) { fprintf(stderr, "rslvq: data row %ld carries label %s, which no codebook row carries\n", s, find_conv_to_lab(l)); goto end; }
    }
  }
  if (pout) pown = malloc(sizeof *pown * (size_t)io.data->num_entries);
  set_teach_params(&params, io.codes, io.data, NULL);
  params.alpha = alpha;
  {
    double *cost = lines && epochs ? calloc((size_t)epochs, sizeof *cost) : NULL, final_cost = 0.0;
    int64_t *correct = lines && epochs ? calloc((size_t)epochs, sizeof *correct) : NULL, final_correct = 0;
    if (!rslvq_training(&params, epochs, sigma2, cost, correct, &final_cost, &final_correct, pown)) {
      for (long t = 0; lines && t < epochs; t++) {
        const float a = alpha * (float)(epochs - t) / (float)epochs;   /* the engine's alpha_t */
        fprintf(stdout, "epoch %ld alpha %.9g cost %.17g accuracy %.2f %%\n", t, (double)a, cost[t],
                100.0 * (double)correct[t] / (double)io.data->num_entries);
      }
      fprintf(stdout, "final cost %.17g accuracy %.2f %%\n", final_cost, 100.0 * (double)final_correct / (double)io.data->num_entries);
      error = 0;
      if (epochs > 0) {
        ifverbose(2) fprintf(stderr, "Codebook entries are saved to file %s\n", cout);
        error = save_entries(io.codes, cout) ? 1 : 0;
      }
      if (!error && pout) error = write_pown(pout, io.data, pown);
    }
    free(cost);
    free(correct);
  }
end:
  free(pown);
  close_entries(io.data);
  close_entries(io.codes);
  pak_shutdown();
  return error;
}
