/* mplx_wait.h -- wait edges: "stand still for one primitive" as a successor.  get_succ drops the successor that equals
 * its parent (reference env_map.h:158, compared without t), so the lists of mplx_expand_lists_device never hold it.  In
 * a table with time keys (include/mplx_table.h) the node (state, t + dt) is another node than (state, t), and a search
 * among reservations (include/mplx_reserve.h) needs the edge between them: a robot that lets another pass waits.
 * mplx_lists_add_wait_device appends that edge to the lists of an expansion, between the expansion and the check.
 * Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.  The reference has nothing of the
 * kind; what is normative is stated here and restated sequentially in tests/wait_model.py.
 *
 * All arithmetic is IEEE double under -ffp-contract=off, in the order written.
 *
 * The zero action.  a0 = the smallest index of a row of the context's control table whose every entry is == 0.0 (the
 *   yaw rate included; -0.0 counts).  It is found on the host when the call is made; without one: MPLX_ERR_STATE.
 *
 * Eligibility.  Row k < n_nodes of the lists belongs to parent state k (field-major [4D+2][parent_stride]: the frontier
 *   that was expanded).  A row with d_parent_id[k] < 0 is skipped (d_parent_id == NULL: no row is).  Otherwise the pair
 *   (parent state k, U[a0]) is evaluated as every pair of get_succ is (the functions of the expansion: the primitive,
 *   the successor state tn = pr.evaluate(dt), both lattice hashes, validate_yaw at both ends where yaw_max > 0 applies
 *   -- with the device's cos / sin, as mplx_rollout_device decides it --, the limits v_max / a_max / j_max).  The row
 *   gets a wait entry iff
 *     h_next == h_curr                   (exactly the successor the reference dropped for tn == curr),
 *     the pair is valid,
 *     cpos[i] == npos[i] on every axis   (the position does not move at all: env_map.h:163 gives the traversal cost 0
 *                                         and no map cell is read),
 *     count[k] < S                       (S = node_stride; with a complete control table it always holds: a0 itself was
 *                                         skipped by the expansion).
 *   A velocity below the lattice resolution keeps the hash but moves the position: no wait entry.
 *
 * The entry is written at e = k * S + count[k], then count[k] += 1:
 *     action[e] = a0
 *     cost[e]   = 0 + (J + w * dt), J the control effort of the zero control summed over the axes from 0 (the expression
 *                 of env_map.h:164-165 for a traversal cost of 0)
 *     hash[e]   = h_next
 *     state     rows of tn (pos, vel, acc, jrk, yaw), the t row = tp + dt (one IEEE add, env_map.h:161)
 *     heur / flags[e]  exactly as mplx_post_lists_device states them for that hash and state, with the goal of
 *                 mplx_set_goal (either row without a goal: MPLX_ERR_STATE)
 *     iters[e]  = 0
 *   Only the rows that are non-NULL are written.  No other byte of the lists changes, entries past the new count
 *   included.  The wait entry is the LAST of its list: lists otherwise ascend in control index, and after this call a
 *   list may end with a0 out of order.  The tie rule of mplx_table_relax_device (the smallest entry index) therefore
 *   lets a wait lose every tie.  A state row that the control can only fill with +0.0 (the derivative rows above the
 *   control order, the yaw row without yaw controls) receives +0.0: a `zero_rows` mask the caller carries for the buffer
 *   (include/mplx.h) stays true, and the caller keeps it.
 *
 * *d_n_added (optional, one int64) grows by the entries added.  Every output is written by the one lane that owns the
 * row.  The call first lets the context finalise the pending heading-limit decisions of an expansion with yaw controls,
 * as mplx_table_relax_device and mplx_reserve_check_device do, then runs asynchronously on the context's stream with no
 * host read.  The check of include/mplx_reserve.h tests a wait edge with its unchanged arithmetic: a zero control from
 * rest evaluates to a constant position.
 *
 * What the rest of the library makes of a wait: mplx_rollout and MapPlanner::checkTraj stop at it with
 * MPLX_SLOT_SKIP_SAME (they are get_succ's arithmetic); mplx_traj_info / _sample / _traverse / _conflicts take the chain
 * as it is.
 *
 * Errors: MPLX_ERR_ARG for NULL ctx / lists / parent states, n_nodes < 0, lists without count / action / cost,
 * node_stride < 1, more than 2^31 - 2 list entries, parent_stride < n_nodes, a state row with state_stride < n_nodes * S;
 * MPLX_ERR_STATE without params / controls, without a zero row in the control table, and for heur / flags without a
 * goal.  n_nodes == 0 is a no-op (after the checks). */
#ifndef MPLX_WAIT_H
#define MPLX_WAIT_H

#include "mplx.h"

#ifdef __cplusplus
extern "C" {
#endif

int mplx_lists_add_wait_device(mplx_ctx *ctx, const mplx_succ_lists *d_lists, int64_t n_nodes, const double *d_parent_state,
                               int64_t parent_stride, const int32_t *d_parent_id_or_null, int64_t *d_n_added_or_null);

#ifdef __cplusplus
}
#endif
#endif
