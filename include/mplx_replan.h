/* mplx_replan.h -- re-rooting and repair of a node table (include/mplx_table.h, include/mplx_multi.h) after the robot
 * has moved along its path and the map has been edited: what of the table is still valid is kept, with its g values,
 * and handed back as one frontier; everything else returns to the state of a node that was never reached.  The
 * reference answers the same need with LPA* (getSubStateSpace, updateBlockedNodes / updateClearedNodes); a table keeps
 * only the best predecessor, so the rule here is "keep the tree below the new root whose edges still hold and expand
 * all of it again in one round".  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * The rule works on the table's n nodes as they are when the call is reached: g, pred and pred_action are a snapshot.
 *
 * Root.  Let r_q be the root given for the query q of node id (mplx_table_rebase_device: root_id, q = 0;
 * mplx_table_rebase_multi_device: d_root_of_query[q]).
 *   r_q >= 0:  root(id) iff id == r_q, id belongs to query q and g[id] is finite;
 *   otherwise: root(id) iff pred[id] == -1 and g[id] is finite (the seeds).
 * An r_q that is out of range, belongs to another query or has an infinite g makes no root: nothing of q is kept then,
 * and that is no error.
 *
 * Bad edge.  bad(id) is defined for a non-root id with p = pred[id] >= 0, and only when check_edges != 0.  The ONE pair
 * (state[p], U[pred_action[id]]) is evaluated on the maps (occupancy, potential, search region) and the parameters the
 * context holds NOW, exactly as a step of mplx_rollout_device evaluates it.  id is bad iff
 *   pred_action[id] is outside [0, nU),  or
 *   the slot status is not MPLX_SLOT_FINITE,  or
 *   the successor's lattice hash differs from hash[id],  or
 *   g[p] + cost > g[id]  (one IEEE add).
 * The last test is > on purpose: a child whose parent improved after the child was relaxed last is merely stale, and its
 * g is still the cost of a path that exists.  With check_edges == 0 no edge is bad -- with one exception that holds
 * whatever check_edges is: a non-root id whose pred[id] >= n names no node of the table; its edge is bad and counted in
 * n_bad_edges, and neither state[pred[id]] nor any other row past n is read.
 * With yaw controls and a heading limit, a pair with a heading-limit decision inside the band of the yaw pinning (what
 * mplx_rollout_device reports as MPLX_ROLLOUT_HEADING_BAND) counts as bad: the decision is taken with the device's
 * cos / sin, which may differ from the host libm's in the last place, and is not trusted near its threshold.  Dropping a
 * valid node is always safe -- the expansion of the kept nodes that follows a rebase goes through the pinned lists and
 * finds the node again -- while keeping an invalid one is not.
 *
 * Kept.  kept(id) is the least fixed point of  root(id) || (pred[id] >= 0 && !bad(id) && kept(pred[id])).  A chain
 * that never reaches a root is not kept: a seed that is not a root, a node whose g was never lowered, a cycle of
 * predecessors (none should exist; the rule is bounded all the same).
 *
 * Apply.  A node that is not kept gets g = +inf and pred = pred_action = -1: the state mplx_table_relax_device gives a
 * node it has just created.  A kept root gets pred = pred_action = -1 and keeps its g, so costs go on being measured
 * from the original start (StateSpace::start_g_).  hash, state, the query column, the hash table's slots and the
 * number of nodes are untouched: nothing is renumbered and the ids a caller holds stay valid.
 *
 * Frontier.  The kept nodes go to d_kept in ascending id as id, g and the state rows gathered from the table -- the
 * layout mplx_table_relax_device emits -- with *count = n_kept.  A frontier smaller than that raises
 * MPLX_TABLE_FRONTIER_FULL with the consequences include/mplx_table.h states.  Rows past the count are not written.
 *
 * Result.  n_kept; n_bad_edges = the non-root nodes with pred >= 0 that are bad; n_roots.
 *
 * Every output is a pure function of the inputs.  No call loops without bound or writes past an array: the closure is
 * computed by pointer doubling over pred, ceil(log2(bound of n_nodes)) + 1 passes, and whatever is undecided after them
 * (a cycle) is dropped.  The passes' scratch belongs to the table and is allocated on the first call.
 *
 * mplx_open_push_closed_device is mplx_open_push_device (include/mplx_open.h, include/mplx_multi.h) in every word of
 * its specification, the ray trace and the per-query goals included, except that
 *   flags[id] = SEEN | (goal ? IS_GOAL : 0)
 * -- the row's key and goal bit are set, and the node is closed.  It gives the kept nodes of a rebase their keys, so
 * that a kept node inside the goal region takes part in the stopping rule of a select, without opening them.
 *
 * All three calls are asynchronous on the context's stream; h_result_or_null != NULL costs one synchronisation.
 *
 * Errors: MPLX_ERR_ARG for NULL required pointers, root_id < -1 and a frontier without id / g / state / count or with
 * state_stride < capacity or capacity < 0; MPLX_ERR_STATE for a table with a status bit (calls queued before the host
 * saw the bit do nothing), for check_edges != 0 without map, parameters or controls, and for mplx_table_rebase_device
 * on a table with Q > 1, and for either rebase on a table with time keys (mplx_table_set_time_keys: the identity test here
 * compares lattice hashes, and nothing here knows wait edges or reservations; mplx_table_rebase_timed_device of
 * include/mplx_replan_timed.h rebases such a table -- its kept nodes go on measuring t, like g, from the original start).
 * A table without nodes is a successful no-op with count 0.  mplx_table_rebase_multi_device
 * accepts a table of one query and then gives the bytes of the plain call.                                           */
#ifndef MPLX_REPLAN_H
#define MPLX_REPLAN_H

#include "mplx_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int64_t n_kept, n_bad_edges, n_roots;
} mplx_rebase_result;

/* The table of one query; root_id = -1: the roots are the seeds.                                                    */
int mplx_table_rebase_device(mplx_table *tab, int32_t root_id, int32_t check_edges, const mplx_table_frontier *d_kept,
                             mplx_rebase_result *d_result_or_null, mplx_rebase_result *h_result_or_null);
/* d_root_of_query: [Q] in device memory, -1 per query = that query's seeds.                                         */
int mplx_table_rebase_multi_device(mplx_table *tab, const int32_t *d_root_of_query, int32_t check_edges,
                                   const mplx_table_frontier *d_kept, mplx_rebase_result *d_result_or_null,
                                   mplx_rebase_result *h_result_or_null);
/* mplx_open_push_device without IS_OPEN.                                                                            */
int mplx_open_push_closed_device(mplx_open *o, const mplx_table_frontier *d_rows, int64_t n_max, double eps, int32_t sight);

#ifdef __cplusplus
}
#endif
#endif
