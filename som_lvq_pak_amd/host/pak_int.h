/* pak_int.h -- what the units of the tools' host library share with each other: pak_engine.c (one GPU) and
 * pak_ranks.c (one process per GPU) over pak_io.c (no GPU).  Included by those units only, never by a tool:
 * pak.h is the tools' API. */
#ifndef PAK_INT_H
#define PAK_INT_H

#include "pak.h"

/* the process's one engine, made on first use on device pak_device; NULL after a message */
somhip_engine *pak_engine(void);
int pak_engine_is_open(void);           /* 1 once pak_engine() has made it (the ranks must be forked before that) */
extern int pak_device;                  /* a rank of a multi-GPU run sets this before its first pak_engine() */

/* device mirrors of host rows; with_labels: the rows' first labels go along.  NULL after a message */
int32_t *pak_first_labels(struct entries *e);      /* [num_entries], malloc'd */
somhip_codebook *pak_mirror_codes(struct entries *codes, int with_labels);
somhip_dataset *pak_mirror_data(struct entries *data, int with_labels);
/* rows [first, first + count) alone: uploaded, or -- a gen: source -- generated in place from `first`; with_labels: with
 * the first labels of the host rows (a labelled gen: source has them: pak_io.c makes its rows and labels on the host
 * when it is opened) */
somhip_dataset *pak_mirror_rows(struct entries *data, long first, long count, int with_labels);

/* What every training entry point refuses before it touches a GPU, with the messages under the caller's prefix
 * `who`: no data, always; PAK_CHECK_SOM: a lattice set_som_params refuses, code dimension != data dimension;
 * PAK_CHECK_RANKS (the -gpus paths): -buffer with -rand, and the notice that snapshots are not written.
 * 0, or 1 after the message. */
#define PAK_CHECK_SOM 1
#define PAK_CHECK_RANKS 2
int pak_check_inputs(struct teach_params *teach, const char *who, int what);

/* rows first .. first+n-1 in the order the running orand() shuffles them into (malloc'd): -rand, and -buffer's feed */
long *pak_shuffled_rows(long first, long n);

#endif
