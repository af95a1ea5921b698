/* mplx_anytime.h -- re-key an open set and bound its result: what an anytime planner (ARA*) does between two searches on
 * one tree.  Every key of include/mplx_open.h is f = g + eps * h, and only the keys depend on eps: the table keeps g, hash
 * and the state rows, the open set keeps which nodes are open.  This call recomputes the keys of all nodes of the table
 * for another eps, and reports per query the smallest g + h among its open nodes -- the number a suboptimality bound is
 * made from.  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.  Nothing here changes
 * a push or a select.
 *
 * mplx_open_rekey_device.  The sequential rule, for every id in [0, n_nodes) of the table whose flags have MPLX_OPEN_SEEN,
 * in any order, with q the node's query (0 on a table of one query):
 *   h       exactly what mplx_open_push_device computes for a frontier row that holds the node: from the table's hash[id],
 *           the state rows gathered from the table (the time row for priors), the goal of q (mplx_set_goal, or
 *           mplx_open_set_goals) and every mode the open set has on -- priors (include/mplx_prior.h), a goal field
 *           (include/mplx_field.h), mplx_open_set_heur(ROBUST) (include/mplx_heur.h); the goal's own lattice state keeps
 *           h = 0.  Bit for bit the h of a push.
 *   L       = g[id] + h: one add, never contracted; g is the table's current value.
 *   bound   if the node has MPLX_OPEN_IS_OPEN: n_open[q] += 1, and if L >= 0 (not a NaN): lower[q] = min(lower[q], L).
 *           n_open counts the open nodes before any pruning.  lower[q] = +inf when no open node of q has such an L.
 *   write != 0:
 *     f     = g[id] + eps * h: one multiply and one add, never contracted; for eps == 0, f = g[id]; -0.0 becomes +0.0 as
 *           in the push.  If f >= 0: f[id] = f and n_rekeyed[q] += 1.  Otherwise (a NaN) the node keeps its key and is
 *           not counted.
 *     flags are not touched, but for pruning: IS_GOAL does not depend on eps, and neither the ray trace of a push with
 *           sight nor the park veto of a reservation table is run again.
 *     h_cut_or_null != NULL and cut[q] < +inf: an open node with L >= cut[q] loses MPLX_OPEN_IS_OPEN and n_pruned[q] += 1.
 *           A tie is pruned; cut[q] = +inf prunes nothing, whatever L is; a NaN L is never pruned.
 *   write == 0: no byte of f or flags changes; h_cut is checked and otherwise ignored.  The call is the bound alone.
 * A node that was pushed with the table's current g[id], the goal and the modes in force and this eps keeps its key bit
 * for bit: after a search, a re-key with the search's own eps changes nothing.
 *
 * The bound goes to d_bound_or_null (device memory, [n_queries]) and, with h_bound_or_null != NULL, to the host: the
 * call's one read-back, with one synchronisation, as h_result of a select.  Without h_cut and without h_bound the call
 * is asynchronous on the context's stream.  h_cut is host memory: it is copied into a buffer of the open set's own (not
 * the context's staging arena, so the call shares no memory with other host-pointer calls), and a call with h_cut
 * synchronises before it returns.
 *
 * Cost: three launches (one lane per query, one lane per node of the table, one lane per query), none of which waits for
 * the host.  An open set's first re-key allocates 32 (with a cut 40) bytes of device memory and 32 bytes of pinned host memory per query,
 * freed with the open set.
 *
 * Errors, as in include/mplx_open.h: MPLX_ERR_ARG for NULL o, an eps that is negative, NaN or infinite, and a cut with a
 * NaN or a negative entry; MPLX_ERR_STATE for a table with a status bit (launches queued before the host saw the bit
 * return at their first instruction; f, flags and the bound are then as they were), for no goal, and for a goal field in
 * force that is stale or was destroyed, and every other state a push refuses.  A call that fails changes nothing.  A table
 * without nodes is a successful no-op with lower = +inf and all counts 0.  No call writes past any array or loops without
 * bound.                                                                                                             */
#ifndef MPLX_ANYTIME_H
#define MPLX_ANYTIME_H

#include "mplx_open.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { double lower; int64_t n_open, n_pruned, n_rekeyed; } mplx_open_bound;   /* one per query */

int mplx_open_rekey_device(mplx_open *o, double eps, int32_t write,
                           const double *h_cut_or_null,          /* [n_queries] */
                           mplx_open_bound *d_bound_or_null,     /* device, [n_queries] */
                           mplx_open_bound *h_bound_or_null);    /* host,   [n_queries]: the call's one read-back */

#ifdef __cplusplus
}
#endif
#endif
