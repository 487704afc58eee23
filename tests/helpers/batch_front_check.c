/* batch_front_check.c -- the batch tools' shared front end (pak_io.c, linked alone with -lm), the functions of it that
 * return rather than exit: made to run under AddressSanitizer / UBSan as well as plain.
 *
 *   batch_front_check data.dat codes lacking.cod    (labelled files: `codes` carries every label of the data, and
 *                                                    lacking.cod does not)
 *
 *   pak_labelled_inputs, pak_masked_inputs    on the two pairs, and on small files written here with each defect; what
 *                                             they say goes to a file, is compared with the message expected (for
 *                                             lacking.cod: any message) and reported
 *   pak_linear_rate, pak_linear_radius        against the written-out expressions, as bit patterns, for epochs 1, 2, 3
 *                                             and 1000 and every t
 *   pak_print_epoch_costs, _final_cost        into a file that is read back
 *   pak_save_codes                            the saved file opens again with its rows
 *
 * One line per check on stdout, "failed checks N" last; exit status = N != 0.  Files are written into the current
 * directory. */
#include <fcntl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "pak.h"

static int failures = 0;
static void check(int ok, const char *what)
{
  printf("%s %s\n", ok ? "ok" : "FAILED", what);
  failures += !ok;
}

static void write_file(const char *name, const char *text)
{
  FILE *fp = fopen(name, "w");
  fputs(text, fp);
  fclose(fp);
}
static char *read_file(const char *name)
{
  static char text[4096];
  FILE *fp = fopen(name, "r");
  const size_t n = fp ? fread(text, 1, sizeof text - 1, fp) : 0;
  if (fp) fclose(fp);
  text[n] = 0;
  return text;
}

/* stderr into said.txt while a check speaks, and back: the test wants the program's own stderr empty */
static int kept = -1;
static void listen(void)
{
  fflush(stderr);
  kept = dup(2);
  const int fd = open("said.txt", O_WRONLY | O_CREAT | O_TRUNC, 0600);
  dup2(fd, 2);
  close(fd);
}
static const char *said(void)
{
  fflush(stderr);
  dup2(kept, 2);
  close(kept);
  return read_file("said.txt");
}

/* both checks, masks first as the tools call them, on the pair (cin, din): the status and the message expected (NULL: any) */
static const char *base(const char *path) { const char *s = strrchr(path, '/'); return s ? s + 1 : path; }
static void inputs(const char *cin, const char *din, const char *data_tail, int want, const char *message)
{
  struct pak_inputs io;
  char what[512];
  listen();
  int rc = pak_open_inputs(din, 0, "cant open data file '%s'\n", cin, 0, "Can't open code file '%s'\n", 0, &io);
  if (rc) { said(); check(0, base(cin)); return; }
  rc = pak_masked_inputs("tool", &io, cin, din, data_tail) || pak_labelled_inputs("tool", &io, cin, din);
  const char *text = said();
  snprintf(what, sizeof what, "inputs %s %s -> %d %s", base(cin), base(din), rc, *text && !strchr(text, '/') ? text : "\n");
  what[strlen(what) - 1] = 0;
  check(rc == want && (message ? strcmp(text, message) == 0 : *text != 0), what);
  close_entries(io.data);
  close_entries(io.codes);
}

static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
  if (argc != 4) { fprintf(stderr, "usage: batch_front_check data.dat codes lacking.cod\n"); return 2; }
  {                                                        /* -v: absent, bare, bare before an option, with a level */
    char *none[] = {"tool", "-din", "f"}, *bare[] = {"tool", "-din", "f", "-v"}, *before[] = {"tool", "-v", "-din", "f"};
    char *level[] = {"tool", "-v", "2", "-din", "f"};
    check(pak_batch_verbose(3, none) == 0 && verbose_level == 1, "no -v: no lines, level 1");
    check(pak_batch_verbose(4, bare) == 1 && verbose_level == 1, "a bare -v: lines, level 1");
    check(pak_batch_verbose(4, before) == 1 && verbose_level == 1, "-v before an option: lines, level 1");
    check(pak_batch_verbose(5, level) == 1 && verbose_level == 2, "-v 2: lines, level 2");
  }
  verbose_level = 0;
  inputs(argv[2], argv[1], "", 0, "");
  inputs(argv[3], argv[1], "", 1, NULL);

  write_file("lab.cod", "2\n0 0 a\n1 1 b\n1 0 b\n");
  write_file("lab.dat", "2\n0 0.1 a\n1 0.9 b\n0.2 0 a\n0.9 0.2 b\n");
  write_file("nolab.cod", "2\n0 0 a\n1 1\n1 0 b\n");
  write_file("nolab.dat", "2\n0 0.1 a\n1 0.9 b\n0.2 0\n0.9 0.2 b\n");
  write_file("one.cod", "2\n0 0 a\n1 1 a\n1 0 a\n");
  write_file("unk.dat", "2\n0 0.1 a\n1 0.9 b\n0.2 0 c\n0.9 0.2 d\n");
  write_file("x.cod", "2\n0 0 a\nx 1 b\n1 0 b\n");
  write_file("x.dat", "2\n0 0.1 a\n1 x b\n0.2 0 a\n0.9 0.2 b\n");
  inputs("lab.cod", "lab.dat", "", 0, "");
  inputs("nolab.cod", "nolab.dat", "", 1, "tool: codebook nolab.cod has no labels on row 1\n");
  inputs("lab.cod", "nolab.dat", "", 1, "tool: data nolab.dat has no labels on row 2\n");
  inputs("one.cod", "nolab.dat", "", 1, "tool: data nolab.dat has no labels on row 2\n");
  inputs("one.cod", "unk.dat", "", 1, "tool: every row of codebook one.cod carries one label (no other class to be wrong with)\n");
  inputs("lab.cod", "unk.dat", "", 1, "tool: data row 2 carries label c, which no codebook row carries\n");
  inputs("x.cod", "x.dat", "", 1, "tool: codebook x.cod has masked components (x): not supported\n");
  inputs("x.cod", "nolab.dat", NULL, 1, "tool: codebook x.cod has masked components (x): not supported\n");
  inputs("lab.cod", "x.dat", "", 1, "tool: data x.dat has masked components (x): not supported\n");
  inputs("lab.cod", "x.dat", " without -missing", 1, "tool: data x.dat has masked components (x): not supported without -missing\n");
  inputs("lab.cod", "x.dat", NULL, 0, "");                  /* masked data are taken where no tail is given */

  /* the rates: the expressions the tools and the library wrote out, -ffp-contract=off or not (nothing here can fuse:
   * the product is divided, and the sum's other term is a constant) */
  const long lengths[4] = {1, 2, 3, 1000};
  const float starts[4] = {0.0f, 0.05f, 3.0f, 1.7e-5f};
  long differ = 0, rates = 0;
  for (int l = 0; l < 4; l++)
    for (int k = 0; k < 4; k++)
      for (long t = 0; t < lengths[l]; t++, rates++) {
        const long epochs = lengths[l];
        const float a = starts[k], r = 1.0f + starts[k];
        const float rate = a * (float)(epochs - t) / (float)epochs;
        const float radius = 1.0f + (r - 1.0f) * (float)(epochs - t) / (float)epochs;
        differ += bits_of(pak_linear_rate(a, epochs, t)) != bits_of(rate);
        differ += bits_of(pak_linear_radius(r, epochs, t)) != bits_of(radius);
      }
  printf("rates %ld each, %ld differ\n", rates, differ);
  check(differ == 0, "the rates have the bits of the written-out expressions");
  check(pak_linear_rate(0.05f, 7, 0) == 0.05f && pak_linear_radius(3.0f, 7, 0) == 3.0f, "epoch 0 starts at the value given");

  /* the report lines */
  const double cost[3] = {0.5, 0.1234567890123456789, -1.0 / 3.0};
  const int64_t correct[3] = {0, 5, 7};
  const float eps = 0.25f;
  FILE *fp = fopen("lines.txt", "w");
  pak_print_epoch_costs(fp, 3, 0.75f, NULL, cost, correct, 7);
  pak_print_epoch_costs(fp, 3, 0.75f, &eps, cost, correct, 7);
  pak_print_epoch_costs(fp, 3, 0.75f, &eps, NULL, NULL, 7);          /* no lines were asked for */
  pak_print_final_cost(fp, cost[1], 6, 7);
  fclose(fp);
  char want[1024];
  int n = 0;
  for (int with_eps = 0; with_eps < 2; with_eps++)
    for (long t = 0; t < 3; t++) {
      const float a = 0.75f * (float)(3 - t) / (float)3, e = eps * (float)(3 - t) / (float)3;
      n += snprintf(want + n, sizeof want - n, "epoch %ld alpha %.9g ", t, (double)a);
      if (with_eps) n += snprintf(want + n, sizeof want - n, "eps %.9g ", (double)e);
      n += snprintf(want + n, sizeof want - n, "cost %.17g accuracy %.2f %%\n", cost[t], 100.0 * (double)correct[t] / 7.0);
    }
  snprintf(want + n, sizeof want - n, "final cost %.17g accuracy %.2f %%\n", cost[1], 100.0 * 6.0 / 7.0);
  const char *lines = read_file("lines.txt");
  fputs(lines, stdout);
  check(strcmp(lines, want) == 0, "the report lines are the tools' formats");

  /* the save: silent below -v 2, one line at -v 2, and the file opens again */
  struct entries *codes = open_entries("lab.cod", 0, 1);
  listen();
  int rc = pak_save_codes(codes, "saved.cod");
  check(rc == 0 && strcmp(said(), "") == 0, "pak_save_codes says nothing at -v 0");
  verbose_level = 2;
  listen();
  rc = pak_save_codes(codes, "saved.cod");
  check(rc == 0 && strcmp(said(), "Codebook entries are saved to file saved.cod\n") == 0, "pak_save_codes names the file at -v 2");
  verbose_level = 0;
  struct entries *again = open_entries("saved.cod", 0, 1);
  check(again && again->num_entries == codes->num_entries && again->dimension == codes->dimension &&
        memcmp(again->points, codes->points, sizeof(float) * (size_t)codes->num_entries * codes->dimension) == 0, "the saved codebook opens again");
  close_entries(again);
  close_entries(codes);

  printf("failed checks %d\n", failures);
  return failures != 0;
}
