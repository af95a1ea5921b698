/* mplx_best.h -- the k best open nodes per query: the selection of include/mplx_open.h and include/mplx_multi.h with a
 * bound on the batch.  Their rule takes every open node with f <= f_min + delta, whatever their number, and cuts at the
 * frontier's capacity by id; this one takes the k smallest keys among them, as a priority queue hands them out.  Exported
 * by libmplx.so next to include/mplx.h, whose ABI version it does not change.  Nothing here changes the plain selects.
 *
 * mplx_open_select_best_device / mplx_open_select_best_multi_device.  Per query q:
 *   f_min, goal_f, goal_id, goal_g and status are exactly those of mplx_open_select[_multi]_device: the stopping rule
 *   is untouched, the goal is announced once no open key is below the best goal-region node's.
 *   With status MPLX_OPEN_SELECTED let C = the open nodes of q with f <= T = f_min + delta (one add; +inf allowed).
 *     |C| <= k   the selected set is C
 *     otherwise  the k first members of C in the order (bit pattern of f as uint64, id): everything below the k-th key
 *                F* and, of the nodes at F*, the `ties` smallest ids that fill the remainder.
 *   The union over the SELECTED queries goes to d_out in ascending global id and is cut at d_out->capacity in that
 *   order, exactly as in the plain selects; the nodes not emitted stay open.  count, n_open (open after the call),
 *   *d_out->count, the rows of d_out, FOUND and EMPTY are as in the two headers.  Every output is a pure function of the
 *   inputs.  Keys are ordered by bit pattern, as the existing passes order them (a push stores no -0.0).
 *
 * Equivalence.  A call whose k is at least every query's |C| leaves the frontier, the flags, f and the results byte for
 * byte as the plain select of the same delta does.  The multi form on a table of one query gives the bytes of the plain
 * form.  Either form may follow the other and the plain selects on the same open set.
 *
 * Cost.  A plain select is four launches (five with several queries); a best-select queues the reduce pass, eight
 * histogram passes of 8 bits, three passes that classify and rank, and the tail of the multi select: 15 launches and
 * one memset, none of which waits for the host.  The histogram passes start at the highest bit in which f_min and T
 * differ and end when a query's candidates are no more than k, when a bucket's end falls on k, or at the last digit; the
 * passes no query needs return at their first instruction.
 *
 * Scratch.  An open set's first best-select allocates 64 + Q * (8512 + 16 * ceil(node_capacity / 4096)) bytes of device
 * memory (Q the table's queries: 8 histograms of 256 counters, the states of the passes, a counter per query and 1024
 * ids), freed with the open set.
 *
 * Errors: MPLX_ERR_ARG for k < 1; every error of the plain selects (MPLX_ERR_ARG for NULL required pointers, delta < 0 or
 * NaN, a frontier without id / g / state / count or with state_stride < capacity or capacity < 0; MPLX_ERR_STATE for a
 * table with a status bit); MPLX_ERR_STATE for the single form on a table with Q > 1.  A call that fails leaves the open
 * set as it was.  A frontier of capacity 0 selects nothing and is no error.                                           */
#ifndef MPLX_BEST_H
#define MPLX_BEST_H

#include "mplx_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

int mplx_open_select_best_device(mplx_open *o, int64_t k, double delta, const mplx_table_frontier *d_out,
                                 mplx_open_result *d_result_or_null, mplx_open_result *h_result_or_null);
/* d_results_or_null / h_results_or_null: Q results each.                                                            */
int mplx_open_select_best_multi_device(mplx_open *o, int64_t k, double delta, const mplx_table_frontier *d_out,
                                       mplx_open_result *d_results_or_null, mplx_open_result *h_results_or_null);

#ifdef __cplusplus
}
#endif
#endif
