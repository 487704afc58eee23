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

/* 1 after a message when a row of e has no label */
static int unlabelled(struct entries *e, const char *what, const char *name)
{
  for (long r = 0; r < e->num_entries; r++)
    if (get_entry_label(&e->rows[r]) == LABEL_EMPTY) {
      fprintf(stderr, "grlvq: %s %s has no labels on row %ld\n", what, name, r);
      return 1;
    }
  return 0;
}

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
  int lines = extract_parameter(argc, argv, "-v", OPTION2) != NULL;
  global_options(argc, argv);
  char *level = extract_parameter(argc, argv, "-v", OPTION);
  if (lines && (!level || level[0] == '-')) verbose_level = 1;   /* a bare -v: the next argument is no level */
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
  if (!(alpha >= 0.0f)) { fprintf(stderr, "grlvq: -alpha %g is negative or not a number\n", (double)alpha); exit(1); }
  if (!(eps >= 0.0f)) { fprintf(stderr, "grlvq: -eps %g is negative or not a number\n", (double)eps); exit(1); }
  if (!(beta >= 0.0f)) { fprintf(stderr, "grlvq: -sigmoid %g is negative or not a number\n", (double)beta); exit(1); }

  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (io.codes->masks) { fprintf(stderr, "grlvq: codebook %s has masked components (x): not supported\n", cin); goto end; }
  if (io.data->masks) { fprintf(stderr, "grlvq: data %s has masked components (x): not supported\n", din); goto end; }
  if (unlabelled(io.codes, "codebook", cin) || unlabelled(io.data, "data", din)) goto end;
  {                                                      /* the labels of the two files, before an engine is asked for */
    const long noc = io.codes->num_entries;
    int one = 1;
    for (long r = 1; r < noc; r++) one &= get_entry_label(&io.codes->rows[r]) == get_entry_label(&io.codes->rows[0]);
    if (one) { fprintf(stderr, "grlvq: every row of codebook %s carries one label (no other class to be wrong with)\n", cin); goto end; }
    for (long s = 0; s < io.data->num_entries; s++) {
      const int l = get_entry_label(&io.data->rows[s]);
      long r = 0;
      while (r < noc && get_entry_label(&io.codes->rows[r]) != l) r++;
      if (r == noc) { fprintf(stderr, "grlvq: data row %ld carries label %s, which no codebook row carries\n", s, find_conv_to_lab(l)); goto end; }
    }
  }
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
      for (long t = 0; lines && t < epochs; t++) {
        const float a = alpha * (float)(epochs - t) / (float)epochs;   /* the engine's alpha_t and eps_t */
        const float e = eps * (float)(epochs - t) / (float)epochs;
        fprintf(stdout, "epoch %ld alpha %.9g eps %.9g cost %.17g accuracy %.2f %%\n", t, (double)a, (double)e, cost[t],
                100.0 * (double)correct[t] / (double)io.data->num_entries);
      }
      fprintf(stdout, "final cost %.17g accuracy %.2f %%\n", final_cost, 100.0 * (double)final_correct / (double)io.data->num_entries);
      error = 0;
      if (epochs > 0) {
        ifverbose(2) fprintf(stderr, "Codebook entries are saved to file %s\n", cout);
        error = save_entries(io.codes, cout) ? 1 : 0;
      }
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
