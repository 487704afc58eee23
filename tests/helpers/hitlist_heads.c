/* hitlist_heads.c -- pak_io.c's hit list on label sequences read from a file: one sequence per line, labels separated
 * by blanks (an empty line is an empty sequence).  Per sequence one line "label:freq label:freq ..." -- the whole list,
 * head first, after add_hit of every label in order.  tests/test_knn_vote.py compares it with a Python replay of the
 * reference's list (labels.c:370-410). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pak.h"

int main(int argc, char **argv)
{
  if (argc != 2) { fprintf(stderr, "usage: hitlist_heads file\n"); return 2; }
  FILE *fp = fopen(argv[1], "r");
  if (!fp) { fprintf(stderr, "can't open %s\n", argv[1]); return 2; }
  static char line[1 << 16];
  while (fgets(line, sizeof line, fp)) {
    struct hitlist *h = new_hitlist();
    char *p = line, *end;
    for (;;) {
      long lab = strtol(p, &end, 10);
      if (end == p) break;
      add_hit(h, lab);
      p = end;
    }
    for (long i = 0; i < h->entries; i++) printf("%s%ld:%ld", i ? " " : "", h->label[i], h->freq[i]);
    printf("\n");
    free_hitlist(h);
  }
  fclose(fp);
  return 0;
}
