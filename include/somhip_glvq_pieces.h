/* somhip_glvq_pieces.h -- batch GLVQ (K9) over data in pieces and over the row blocks of ranks: the part of the C ABI of
 * libsomhip.so that continues one epoch of somhip_glvq_train from piece to piece.  include/somhip.h includes this file
 * behind its own declarations (the handles, somhip_glvq_params, somhip_comm and the error convention are there), so a
 * program includes somhip.h alone.  The ctypes mirror is som_lvq_pak_amd/_lib.py GLVQ_PIECES_SIGNATURES;
 * tests/test_glvq_pieces.py holds this header to the checks tests/test_build.py and tests/test_prepared_state.py make of
 * somhip.h: every declaration exported and mirrored, every entry point that takes a codebook checked against the
 * codebook's prepared copies. */
#ifndef SOMHIP_GLVQ_PIECES_H
#define SOMHIP_GLVQ_PIECES_H

#include "somhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- one epoch of batch GLVQ over data in pieces -----------------------------------
 * The sums of step 4 of somhip_glvq_train are chains of fp64 additions in data order, and a chain can be continued: the
 * data of an epoch may come in pieces -- buffers, calls, the row blocks of ranks -- and leave the bits of one call.
 * The state is ONE device blob the codebook owns (not engine scratch: other engine calls between two pieces leave it
 * alone), for a codebook of R rows and dimension d:
 *   [Sp | sp] then [Sm | sm]   2 x R x (d + 1) doubles          (step 4's sums, role + first)
 *   cost                       R doubles
 *   np, nm                     R uint32 each
 *   tail                       { uint64 samples; uint64 correct }   16 bytes
 * It opens as all-zero bits.  Nothing of an accumulation lives on the host between calls, so the blob copied into another
 * codebook of the same shape, whose own state _begin has opened, continues the accumulation there.
 *   _begin       opens, or re-zeroes, the state.
 *   _accumulate  steps 2-4 over rows (first + s) % n_rows, s < n, of ds against the codebook as it stands: the search,
 *                the terms and the grouping of the piece are somhip_glvq_train's own stages (the search route is the plan's
 *                for the piece's n: both routes are exact, so the keys do not depend on it); then every chain goes on
 *                from what the state holds, np / nm grow by the piece's counts and the tail by n and the piece's correct
 *                samples.  Pieces may come from different data sets; each wraps inside its own.
 *   _finish      step 5 with a = (double)alpha_t / (double)samples, samples from the tail; a row with np == nm == 0 keeps
 *                its bits.  *cost_out (or NULL) = (the host's fp64 chain over cost[j] in row order) / samples, the figure
 *                somhip_glvq_train forms; *correct_out, *samples_out (or NULL) from the tail.  After it further pieces,
 *                and a second _finish, are refused ("the codebook has moved") until the next _begin.
 *   _end         frees the state (somhip_codebook_destroy does too).
 *   _state       the blob's device address and size, while a state is open.
 * _begin, _accumulate over the pieces in order, _finish(alpha_t) leave the codebook, the cost and the count with the bits
 * of one epoch of somhip_glvq_train at that alpha_t over a data set whose rows are the pieces' rows in that order.
 * Refused by name before anything is launched, rows and state untouched: everything somhip_glvq_train refuses of a piece
 * (masked data, missing labels, a data label the codebook lacks, a one-class codebook, a sharded codebook, n <= 0,
 * first < 0, another dimension); _accumulate, _finish or _state without _begin; a piece that would take the total to 2^32
 * samples; alpha_t or sigmoid_beta negative or NaN; _finish on a state that holds no sample.  Every other call that
 * writes the codebook's rows (upload, the trainings, the batch map) closes the state.  The launches count under the four
 * ids of somhip_glvq_timing: the continued sums and the counts under [2], the update under [3]. */
int  somhip_glvq_begin(somhip_codebook *cb);
int  somhip_glvq_accumulate(somhip_codebook *cb, somhip_dataset *ds, int64_t first, int64_t n, float sigmoid_beta);
int  somhip_glvq_finish(somhip_codebook *cb, float alpha_t, double *cost_out, int64_t *correct_out, int64_t *samples_out);
int  somhip_glvq_end(somhip_codebook *cb);
int  somhip_glvq_state(somhip_codebook *cb, void **dev_state, int64_t *bytes);

/* ---- the epochs of somhip_glvq_train over the row blocks of G ranks ----------------
 * Every rank holds the whole codebook and a contiguous block of the data's rows (`block`; p->first, p->n describe the
 * rank's own rows, and p->n == 0 -- a rank without rows, block ignored -- is legal here and only here).  Per epoch every
 * rank runs the search, the terms and the grouping on its own block, all ranks at the same time; then, for root =
 * 0 .. G-1, rank root continues the sums from the state it holds and the state is broadcast from it
 * (somhip_comm_broadcast), so after the last turn every rank holds the sums of the whole data in rank order; then every
 * rank runs the same update on the same state -- the same bits everywhere, no gather.  `count` epochs leave on every rank
 * the bits of somhip_glvq_train over the blocks in rank order; cost_out / correct_out ([count] or NULL) are filled on
 * every rank alike.  Before any rank launches anything the blocks' sizes are all-reduced (as two 16-bit halves) and a
 * total of 2^32 or more is refused on every rank alike.  The state is the call's own: closed and freed on every way out. */
int  somhip_glvq_train_ranks(somhip_codebook *cb, somhip_dataset *block, const somhip_glvq_params *p, somhip_comm *c,
                             double *cost_out /*[count] or NULL*/, int64_t *correct_out /*[count] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* SOMHIP_GLVQ_PIECES_H */
