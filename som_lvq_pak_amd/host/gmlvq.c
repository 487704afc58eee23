/* gmlvq -- train a labelled codebook with batch GMLVQ on the MI355X engine (somhip_gmlvq_train): Schneider, Biehl and
 * Hammer's matrix relevance GLVQ as full-batch gradient steps.  It is batch GLVQ (glvq) under d(x, w) = |Omega (x - w)|^2
 * and learns the rank x dim matrix Omega with the rows: the rates go linearly from -alpha and -eps to 0 over -epochs
 * epochs.  -oout writes Omega, -oin reads one, -pout writes the data projected by it; -epochs 0 -oin only evaluates a
 * trained model.  This project's own tool: LVQ_PAK has none. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "pak.h"

static const char *usage =
    "gmlvq - train a labelled codebook and its matrix metric, batch GMLVQ (MI355X engine)\n"
    "Required:  -cin file  -din file  -cout file  -epochs T  -alpha A  -eps E\n"
    "Optional:  -rank M (the rows of Omega, 1 .. dim; without it dim, or the rows of -oin)\n"
    "           -sigmoid B (the cost is 1 / (1 + exp(-B mu)); without it, mu itself)\n"
    "           -oin file (the matrix to start from, taken as it is; without it 1 / sqrt(dim) where k mod M == r)\n"
    "           -oout file (the matrix the run ends with)\n"
    "           -pout file (the data projected by that matrix: a .dat of dimension M with the labels)\n"
    "           -v (one line per epoch to stdout: epoch, alpha, eps, cost and accuracy before it)\n"
    "-epochs 0 with -oin trains nothing and writes no codebook: it prints the cost and accuracy of -cin under -oin.\n"
    "An omega file is a first line 'M dim', then M lines of dim values.\n"
    "-alpha has the unit of a squared distance: about the squared distance between neighbouring classes.\n"
    "Files:     text (.dat/.cod) or raw fp32 (a name ending in .f32; see datconv); every row carries a label\n";

/* the matrix of file `name`: *rank from its first line (which must agree with `want` where that is > 0), the values into a
 * new array *omega; 1 after a message */
static int read_omega(const char *name, int dim, int want, int *rank, float **omega)
{
  FILE *fp = fopen(name, "r");
  char word[64];
  long m = 0, d = 0;
  int rc = 1;
  if (!fp) { fprintf(stderr, "gmlvq: can't open omega file '%s'\n", name); return 1; }
  {
    const int got = fscanf(fp, "%ld %ld", &m, &d);
    if (got == EOF) { fprintf(stderr, "gmlvq: omega file %s is empty\n", name); goto out; }
    if (got != 2) { fprintf(stderr, "gmlvq: omega file %s: can't read 'M dim' from its first line\n", name); goto out; }
  }
  if (d != dim) { fprintf(stderr, "gmlvq: omega file %s has dimension %ld, the codebook %d\n", name, d, dim); goto out; }
  if (m < 1 || m > dim) { fprintf(stderr, "gmlvq: omega file %s has %ld rows, outside 1 .. %d\n", name, m, dim); goto out; }
  if (want > 0 && m != want) { fprintf(stderr, "gmlvq: omega file %s has %ld rows, -rank asks for %d\n", name, m, want); goto out; }
  *omega = malloc(sizeof **omega * (size_t)m * (size_t)dim);
  for (long i = 0; i < m * dim; i++) {
    char *end;
    if (fscanf(fp, "%63s", word) != 1) { fprintf(stderr, "gmlvq: omega file %s ends after %ld of %ld values\n", name, i, m * dim); goto out; }
    const float v = strtof(word, &end);
    if (end == word || *end) { fprintf(stderr, "gmlvq: omega file %s: can't read value %ld ('%s')\n", name, i, word); goto out; }
    if (isnan(v) || isinf(v)) { fprintf(stderr, "gmlvq: omega file %s: value %ld (%g) is not a finite number\n", name, i, (double)v); goto out; }
    (*omega)[i] = v;
  }
  *rank = (int)m;
  rc = 0;
out:
  fclose(fp);
  return rc;
}

/* "%.9g" carries a float through text and back */
static int write_omega(const char *name, int rank, int dim, const float *omega)
{
  FILE *fp = fopen(name, "w");
  if (!fp) { fprintf(stderr, "gmlvq: can't open omega file '%s' for writing\n", name); return 1; }
  fprintf(fp, "%d %d\n", rank, dim);
  for (int r = 0; r < rank; r++)
    for (int k = 0; k < dim; k++) fprintf(fp, "%.9g%c", (double)omega[(size_t)r * dim + k], k + 1 < dim ? ' ' : '\n');
  return fclose(fp) ? 1 : 0;
}

/* the projected data as a .dat of dimension rank, every row with the label of its data row */
static int write_projected(const char *name, struct entries *data, int rank, const float *y)
{
  FILE *fp = fopen(name, "w");
  if (!fp) { fprintf(stderr, "gmlvq: can't open file '%s' for writing\n", name); return 1; }
  fprintf(fp, "%d\n", rank);
  for (long s = 0; s < data->num_entries; s++) {
    for (int r = 0; r < rank; r++) fprintf(fp, "%.9g ", (double)y[(size_t)s * rank + r]);
    fprintf(fp, "%s\n", find_conv_to_lab(get_entry_label(&data->rows[s])));
  }
  return fclose(fp) ? 1 : 0;
}

int main(int argc, char **argv)
{
  struct teach_params params;
  struct pak_inputs io = {NULL, NULL};
  float *omega = NULL, *projected = NULL;
  int error = 1;

  memset(&params, 0, sizeof params);
  int lines = pak_batch_verbose(argc, argv);
  if (extract_parameter(argc, argv, "-help", OPTION2)) { fputs(usage, stdout); exit(0); }
  char *din = extract_parameter(argc, argv, "-din", ALWAYS), *cin = extract_parameter(argc, argv, "-cin", ALWAYS);
  char *oin = extract_parameter(argc, argv, "-oin", OPTION), *oout = extract_parameter(argc, argv, "-oout", OPTION);
  char *pout = extract_parameter(argc, argv, "-pout", OPTION);
  long epochs = oatoi(extract_parameter(argc, argv, "-epochs", ALWAYS), 0);
  char *cout = extract_parameter(argc, argv, "-cout", epochs > 0 ? ALWAYS : OPTION);
  float alpha = oatof(extract_parameter(argc, argv, "-alpha", epochs > 0 ? ALWAYS : OPTION), 0.0f);
  float eps = oatof(extract_parameter(argc, argv, "-eps", epochs > 0 ? ALWAYS : OPTION), 0.0f);
  float beta = oatof(extract_parameter(argc, argv, "-sigmoid", OPTION), 0.0f);
  char *rank_arg = extract_parameter(argc, argv, "-rank", OPTION);
  int rank = (int)oatoi(rank_arg, 0);
  if (epochs < 0) { fprintf(stderr, "gmlvq: -epochs %ld < 0\n", epochs); exit(1); }
  if (epochs == 0 && !oin) { fprintf(stderr, "gmlvq: -epochs 0 evaluates a trained model and needs its matrix (-oin)\n"); exit(1); }
  pak_rate_check("gmlvq", "-alpha", alpha);
  pak_rate_check("gmlvq", "-eps", eps);
  pak_rate_check("gmlvq", "-sigmoid", beta);
  if (rank_arg && rank < 1) { fprintf(stderr, "gmlvq: -rank %s < 1\n", rank_arg); exit(1); }

  if (pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io)) goto end;
  if (pak_masked_inputs("gmlvq", &io, cin, din, "")) goto end;
  if (pak_labelled_inputs("gmlvq", &io, cin, din)) goto end;
  const int dim = io.codes->dimension;
  if (rank > dim) { fprintf(stderr, "gmlvq: -rank %d is larger than the dimension %d\n", rank, dim); goto end; }
  if (oin) { if (read_omega(oin, dim, rank, &rank, &omega)) goto end; }
  else {
    if (!rank) rank = dim;
    omega = calloc((size_t)rank * (size_t)dim, sizeof *omega);
    for (int k = 0; k < dim; k++) omega[(size_t)(k % rank) * dim + k] = (float)(1.0 / sqrt((double)dim));
  }
  if (epochs > 0) {
    int any = 0;
    for (size_t i = 0; i < (size_t)rank * (size_t)dim; i++) any |= omega[i] != 0.0f;
    if (!any) { fprintf(stderr, "gmlvq: the matrix of %s is all zero\n", oin); goto end; }
  }
  if (pout) projected = malloc(sizeof *projected * (size_t)io.data->num_entries * (size_t)rank);
  set_teach_params(&params, io.codes, io.data, NULL);
  params.alpha = alpha;
  {
    double *cost = lines && epochs ? calloc((size_t)epochs, sizeof *cost) : NULL, final_cost = 0.0;
    int64_t *correct = lines && epochs ? calloc((size_t)epochs, sizeof *correct) : NULL, final_correct = 0;
    if (!gmlvq_training(&params, epochs, beta, eps, omega, rank, cost, correct, &final_cost, &final_correct, projected)) {
      pak_print_epoch_costs(stdout, epochs, alpha, &eps, cost, correct, io.data->num_entries);   /* the engine's alpha_t and eps_t */
      pak_print_final_cost(stdout, final_cost, final_correct, io.data->num_entries);
      error = epochs > 0 ? pak_save_codes(io.codes, cout) : 0;
      if (!error && oout) error = write_omega(oout, rank, dim, omega);
      if (!error && pout) error = write_projected(pout, io.data, rank, projected);
    }
    free(cost);
    free(correct);
  }
end:
  free(omega);
  free(projected);
  close_entries(io.data);
  close_entries(io.codes);
  pak_shutdown();
  return error;
}
