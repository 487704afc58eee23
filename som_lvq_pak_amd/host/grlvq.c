/* grlvq -- train a labelled codebook with batch GRLVQ on the MI355X engine (somhip_grlvq_train): Hammer and Villmann's
 * relevance GLVQ as full-batch gradient steps.  It is batch GLVQ (glvq) under d(x, w) = sum_k lambda[k] (x[k] - w[k])^2,
 * and learns the relevances lambda with the rows: the rates go linearly from -alpha and -eps to 0 over -epochs epochs.
 * -rout writes the relevance profile, -rin reads one; -epochs 0 -rin only evaluates a trained model.  This project's own
 * tool: LVQ_PAK has none. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "grlvq - train a labelled codebook and its relevances, batch GRLVQ (MI355X engine)\n"
    "Required:  -cin file  -din file  -cout file  -epochs T  -alpha A  -eps E\n"
    "Optional:  -sigmoid B (the cost is 1 / (1 + exp(-B mu)); without it, mu itself)\n"
    "           -rin file (the relevances to start from, taken as they are; without it 1 / dim each)\n"
    "           -rout file (the relevances the run ends with)\n"
    "           -v (one line per epoch to stdout: epoch, alpha, eps, cost and accuracy before it)\n"
    "-epochs 0 with -rin trains nothing and writes no codebook: it prints the cost and accuracy of -cin under -rin.\n"
    "A relevance file is a first line with the dimension, then one value per line.\n"
    "-alpha has the unit of a squared distance: about the squared distance between neighbouring classes.\n"
    "Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n";

/* the relevances of file `name` into lambda[dim]; 1 after a message */
static int read_relevances(const char *name, int dim, float *lambda)
{
  FILE *fp = fopen(name, "r");
  char line[256], *end;
  int rc = 1;
  if (!fp) { fprintf(stderr, "grlvq: can't open relevance file '%s'\n", name); return 1; }
  if (!fgets(line, sizeof line, fp)) { fprintf(stderr, "grlvq: relevance file %s is empty\n", name); goto out; }
  {
    const long d = strtol(line, &end, 10);
    while (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n') end++;
    if (end == line || *end) { fprintf(stderr, "grlvq: relevance file %s: can't read the dimension from its first line\n", name); goto out; }
    if (d != dim) { fprintf(stderr, "grlvq: relevance file %s has dimension %ld, the codebook %d\n", name, d, dim); goto out; }
  }
  for (int k = 0; k < dim; k++) {
    if (!fgets(line, sizeof line, fp)) { fprintf(stderr, "grlvq: relevance file %s ends after %d of %d values\n", name, k, dim); goto out; }
    const float v = strtof(line, &end);
    while (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n') end++;
    if (end == line || *end) { fprintf(stderr, "grlvq: relevance file %s: can't read value %d\n", name, k); goto out; }
    if (!(v >= 0.0f) || isinf(v)) { fprintf(stderr, "grlvq: relevance file %s: value %d (%g) is negative or not a finite number\n", name, k, (double)v); goto out; }
    lambda[k] = v;
  }
  rc = 0;
out:
  fclose(fp);
  return rc;
}

/* "%.9g" carries a float through text and back */
static int write_relevances(const char *name, int dim, const float *lambda)
{
  FILE *fp = fopen(name, "w");
  if (!fp) { fprintf(stderr, "grlvq: can't open relevance file '%s' for writing\n", name); return 1; }
  fprintf(fp, "%d\n", dim);
  for (int k = 0; k < dim; k++) fprintf(fp, "%.9g\n", (double)lambda[k]);
  return fclose(fp) ? 1 : 0;
}

int main(int argc, char **argv)
{
  struct teach_params params;
  struct pak_inputs io = {NULL, NULL};
  float *lambda = NULL;
  int error = 1;

  memset(&params, 0, sizeof params);
  int lines = pak_batch_verbose(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *din = extract_parameter(argc, argv, "-din", ALWAYS), *cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *rin = extract_parameter(argc, argv, "-rin", OPTION), *rout = extract_parameter(argc, argv, "-rout", OPTION);
  long epochs = oatoi(extract_parameter(argc, argv, "-epochs", ALWAYS), 0);
  char *cout = extract_parameter(argc, argv, "-cout", epochs > 0 ? ALWAYS : OPTION);
  float alpha = oatof(extract_parameter(argc, argv, "-alpha", epochs > 0 ? ALWAYS : OPTION), 0.0f);
  float eps = oatof(extract_parameter(argc, argv, "-eps", epochs > 0 ? ALWAYS : OPTION), 0.0f);
  float beta = oatof(extract_parameter(argc, argv, "-sigmoid", OPTION), 0.0f);
  if (epochs < 0) { fprintf(stderr, "grlvq: -epochs %ld < 0\n", epochs); exit(1); }
  if (epochs == 0 && !rin) { fprintf(stderr, "grlvq: -epochs 0 evaluates a trained model and needs its relevances (-rin)\n"); exit(1); }
  pak_rate_check("grlvq", "-alpha", alpha);
  pak_rate_check("grlvq", "-eps", eps);
  pak_rate_check("grlvq", "-sigmoid", beta);

  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (pak_masked_inputs("grlvq", &io, cin, din, "")) goto end;
  if (pak_labelled_inputs("grlvq", &io, cin, din)) goto end;
  const int dim = io.codes->dimension;
  lambda = malloc(sizeof *lambda * (size_t)dim);
  if (rin) { if (read_relevances(rin, dim, lambda)) goto end; }
  else for (int k = 0; k < dim; k++) lambda[k] = 1.0f / (float)dim;
  if (epochs > 0) {
    double sum = 0.0;
    for (int k = 0; k < dim; k++) sum += (double)lambda[k];
    if (!(sum > 0.0)) { fprintf(stderr, "grlvq: the relevances of %s sum to zero\n", rin); goto end; }
  }
  set_teach_params(&params, io.codes, io.data, NULL);
  params.alpha = alpha;
  {
    double *cost = lines && epochs ? calloc((size_t)epochs, sizeof *cost) : NULL, final_cost = 0.0;
    int64_t *correct = lines && epochs ? calloc((size_t)epochs, sizeof *correct) : NULL, final_correct = 0;
    if (!grlvq_training(&params, epochs, beta, eps, lambda, cost, correct, &final_cost, &final_correct)) {
      pak_print_epoch_costs(stdout, epochs, alpha, &eps, cost, correct, io.data->num_entries);   /* the engine's alpha_t and eps_t */
      pak_print_final_cost(stdout, final_cost, final_correct, io.data->num_entries);
      error = epochs > 0 ? pak_save_codes(io.codes, cout) : 0;
      if (!error && rout) error = write_relevances(rout, dim, lambda);
    }
    free(cost);
    free(correct);
  }
end:
  free(lambda);
  close_entries(io.data);
  close_entries(io.codes);
  pak_shutdown();
  return error;
}
