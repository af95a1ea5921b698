/* mplx_replan_timed.h -- the rebase of include/mplx_replan.h for a search among moving robots: a node table with time
 * keys (include/mplx_table.h), wait edges (include/mplx_wait.h) and a reservation table (include/mplx_reserve.h).
 * Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.  The reference has nothing of the
 * kind; what is normative is stated here and restated sequentially in tests/timed_replan_model.py.
 *
 * Why the untimed rebase refuses such a table, and why this one need not: the robot's clock never has to move.  g goes
 * on being measured from the original start; so does t.  With the t0 of the queries unchanged, t0 + t is still the
 * common clock of include/mplx_conflict.h and the time keys of the kept nodes are still right: nothing is renumbered or
 * re-keyed.  t, the hash column, ids and the t0 of the queries are untouched by the call.
 *
 * mplx_table_rebase_timed_device is mplx_table_rebase_multi_device in every word -- root, kept, apply, frontier, result,
 * errors, purity; a table of one query is accepted, with or without time keys -- except for the definition of a bad
 * edge.  All arithmetic is IEEE double under -ffp-contract=off, in the order written.
 *
 * Take a non-root id with p = pred[id] in [0, n) and a = pred_action[id].  tp = the t row of state[p]; tc = tp + dt (one
 * IEEE add, as include/mplx_reserve.h and include/mplx_wait.h form it).
 *
 * Ordinary edge (check_edges != 0).  As include/mplx_replan.h: the action range, the slot status, the heading band and
 *   g[p] + cost > g[id].  The identity test compares the value the hash column really holds: on a table with time keys
 *   mplx_time_key(h_next, tc), without them h_next.
 * Wait edge (check_edges != 0).  a is the zero action a0 of include/mplx_wait.h and the pair yields the successor
 *   get_succ drops (h_next == h_curr).  With allow_wait != 0 the edge holds iff the eligibility of include/mplx_wait.h
 *   holds (a valid pair, cpos[i] == npos[i] on every axis); its cost is that header's 0 + (J + w * dt); then the same
 *   key test and the same g test.  With allow_wait == 0 such an edge is bad.  Without a zero row in the control table a0
 *   does not exist, no edge is a wait, and that is no error.
 * Reservations (res != NULL, whatever check_edges says).  The edge (state[p], U[a]) is looked at exactly as
 *   mplx_reserve_check_device looks at a finite list entry of a row whose parent is p: the query is the node's own (the
 *   query column; a table of one query: 0), t0 / radius / ignore of mplx_reserve_set_queries, the check's horizon rule,
 *   its closed set of instants, its position (traj::eval_segment, positions only, at s = tl_i - tp) and its strict pair
 *   test.  A conflict, or an edge that leaves the horizon, makes the edge bad.  hit[id] (optional, [node capacity]
 *   int64) = the minimum of ((int64)i << 32 | b) over the edge's conflicts, -2 for the horizon, and -1 for every other
 *   id below n: an edge without a conflict, a root, a node without a predecessor, an action or a predecessor out of
 *   range (bad already, and never read out of range).  Entries at and past n are not written.  *n_blocked (optional, one
 *   int64) grows by the ids with hit != -1.  An edge is tested here whether or not the rules above already made it bad:
 *   the two launches are independent and every output is a minimum or a sum of integers.
 * n_bad_edges counts the union.
 *
 * The call first lets the context finalise pending heading-limit decisions, as mplx_reserve_check_device does, then runs
 * asynchronously on the context's stream; h_result_or_null != NULL costs one synchronisation.
 *
 * Errors: those of mplx_table_rebase_multi_device (without its refusal of time keys), and: MPLX_ERR_ARG for a `res` of
 * another context or with a number of queries other than the table's; MPLX_ERR_STATE for a `res` before a fill or before
 * mplx_reserve_set_queries, and for a `res` without params / controls in the context.  A table without nodes is a
 * successful no-op with count 0 (hit and *n_blocked are not written).                                                 */
#ifndef MPLX_REPLAN_TIMED_H
#define MPLX_REPLAN_TIMED_H

#include "mplx_replan.h"
#include "mplx_reserve.h"
#include "mplx_wait.h"

#ifdef __cplusplus
extern "C" {
#endif

int mplx_table_rebase_timed_device(mplx_table *tab, const int32_t *d_root_of_query, int32_t check_edges, int32_t allow_wait,
                                   mplx_reserve *res_or_null, const mplx_table_frontier *d_kept,
                                   int64_t *d_hit_or_null /* [node capacity] */, int64_t *d_n_blocked_or_null,
                                   mplx_rebase_result *d_result_or_null, mplx_rebase_result *h_result_or_null);

#ifdef __cplusplus
}
#endif
#endif
