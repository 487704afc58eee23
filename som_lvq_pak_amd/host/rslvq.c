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
  int lines = pak_batch_verbose(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *din = extract_parameter(argc, argv, "-din", ALWAYS), *cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *pout = extract_parameter(argc, argv, "-pout", OPTION);
  long epochs = oatoi(extract_parameter(argc, argv, "-epochs", ALWAYS), 0);
  char *cout = extract_parameter(argc, argv, "-cout", epochs > 0 ? ALWAYS : OPTION);
  float alpha = oatof(extract_parameter(argc, argv, "-alpha", epochs > 0 ? ALWAYS : OPTION), 0.0f);
  float sigma2 = (float)atof(extract_parameter(argc, argv, "-sigma2", ALWAYS));
  if (epochs < 0) { fprintf(stderr, "rslvq: -epochs %ld < 0\n", epochs); exit(1); }
  pak_rate_check("rslvq", "-alpha", alpha);
  if (!(sigma2 > 0.0f) || isinf(sigma2)) { fprintf(stderr, "rslvq: -sigma2 %g is not a finite number above 0\n", (double)sigma2); exit(1); }

  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (pak_masked_inputs("rslvq", &io, cin, din, "")) goto end;
  if (pak_labelled_inputs("rslvq", &io, cin, din)) goto end;
  if (pout) pown = malloc(sizeof *pown * (size_t)io.data->num_entries);
  set_teach_params(&params, io.codes, io.data, NULL);
  params.alpha = alpha;
  {
    double *cost = lines && epochs ? calloc((size_t)epochs, sizeof *cost) : NULL, final_cost = 0.0;
    int64_t *correct = lines && epochs ? calloc((size_t)epochs, sizeof *correct) : NULL, final_correct = 0;
    if (!rslvq_training(&params, epochs, sigma2, cost, correct, &final_cost, &final_correct, pown)) {
      pak_print_epoch_costs(stdout, epochs, alpha, NULL, cost, correct, io.data->num_entries);   /* the engine's alpha_t */
      pak_print_final_cost(stdout, final_cost, final_correct, io.data->num_entries);
      error = epochs > 0 ? pak_save_codes(io.codes, cout) : 0;
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
