/* mplx_reserve.h -- a reservation table on the device: the positions of B reserved trajectories at every instant of a
 * common clock, and the check of successor lists against them.  A search that calls the check between its expansion
 * and its relax (include/mplx_table.h) plans among moving robots: prioritised planning is one such search per robot,
 * against the trajectories of the robots planned before it.  Exported by libmplx.so next to include/mplx.h, whose ABI
 * version it does not change.  The reference has nothing of the kind; what is normative is stated here and restated
 * sequentially in tests/reserve_model.py.
 *
 * All arithmetic is IEEE double under -ffp-contract=off, in the order written.
 *
 * Contents.  For B reserved trajectories and n_steps instants at t_i = (double)i * step the table holds pos[i][d][b] and
 *   active[i][b], and per trajectory included[b], radius[b] and group[b]: exactly what the init and position launches
 *   of include/mplx_conflict.h compute for the same set and the same mplx_conflict_in -- the same local time
 *   t_i - t0[b], the same clamp, segment look-up and Lambda, MPLX_CONFLICT_PARK / MPLX_CONFLICT_GONE, the same
 *   exclusion rules (a set status, a t0 that is not finite, a radius that is negative or not finite: excluded, the
 *   latter two with MPLX_CONFLICT_BAD_INPUT in status[b]; an excluded trajectory has radius 0 and blocks nothing) and
 *   group[b] = b without `group`.  The fill IS those launches, on one chunk of n_steps instants; `rank` and
 *   `chunk_steps` of the mplx_conflict_in are ignored.  The table is kept until the next fill or the destroy.
 *   A fill whose positions and active bits, B * n_steps * (8 D + 1) bytes, exceed MPLX_RESERVE_MAX_BYTES (1 GiB) is
 *   MPLX_ERR_ARG.  On the device the positions lie as [D][n_steps][B] (trajectory-minor, as the conflict kernels keep
 *   them); mplx_reserve_positions hands them out as [n_steps][D][B].
 *
 * Queries.  mplx_reserve_set_queries gives, for each of Q planning robots, its start on the clock t0[q] (finite,
 *   >= 0), its radius (finite, >= 0) and a group whose reservations it ignores (-1: none; with it a table that holds
 *   every robot's current plan serves each robot, which skips itself).  The values are copied.
 *
 * Check.  mplx_reserve_check_device looks at the lists of mplx_expand_lists_device (count, action, cost), one row per
 *   expanded node, with parent_id[n_nodes] and the parents' state rows (field-major [4D+2][parent_stride]: the frontier
 *   that was expanded).  The query of row k is query[parent_id[k]] of `tab` when that table has more than one query
 *   (include/mplx_multi.h), else 0.  Entry e = k * S + j IS LOOKED AT iff
 *     j < count[k],  parent_id[k] >= 0,  cost[e] is finite,
 *   and, so that nothing is read out of range: action[e] in [0, nU); on a table with several queries parent_id[k] below
 *   the table's node capacity and its query in [0, Q).  For such an entry, with q its query:
 *     tp = the parent's t row (field 4D+1);  tc = tp + dt (one IEEE add, dt of mplx_set_params);
 *     tl_i = (double)i * step - t0[q].
 *   Horizon.   If (double)(n_steps - 1) * step - t0[q] < tc the edge leaves the table's horizon: it is blocked with hit
 *              -2 and no pair test is made.  Nothing passes unchecked.
 *   Instants.  Otherwise: every i in [0, n_steps) with tl_i >= tp && tl_i <= tc.  Closed at both ends: a boundary instant
 *              belongs to both adjacent edges.  (The kernel starts from a guess and scans at most ceil(dt / step) + 3
 *              instants; tl_i is monotone in i and the set is the one stated, however it is found.)
 *   Position.  At instant i: traj::eval_segment<COMMAND, positions only> at s = tl_i - tp of the segment the chain launch
 *              of include/mplx_traj.h builds from (parent state, U[action[e]]) -- the position mplx_traj_sample gives for
 *              a chain through this edge whose start has t = 0.  Yaw does not enter.
 *   Pair test. Against every b that is included, active at i and has group[b] != ignore[q]: d2 and rr = radius[q] +
 *              radius[b] exactly as the pair test of include/mplx_conflict.h (dx = pos_entry - pos_b); a conflict iff
 *              d2 < rr * rr.  Strict: touching is none.  A d2 that is NaN is no conflict.
 *   Result.    An entry with a conflict (or past the horizon) is BLOCKED: cost[e] = +inf, which every later relax skips.
 *              No other byte of the lists changes.  hit[e] (optional, [n_nodes * S] int64) = the minimum of
 *              ((int64)i << 32 | b) over the entry's conflicts, -2 for the horizon, -1 for an entry without a conflict and
 *              for every entry j < S of the n_nodes rows that is not looked at.  *n_blocked (optional, one int64) is
 *              increased by the number of entries blocked in this call.
 *   Every output is a minimum or a sum of integers: a pure function of the inputs whatever the tiling.
 *
 * The check first lets the context finalise the pending heading-limit decisions of an expansion with yaw controls, as
 * mplx_table_relax_device does (include/mplx_table.h), then runs asynchronously on the context's stream with no host
 * read.  The fills with _device are asynchronous too; the host-pointer twins stage through the context's arena and are
 * synchronous, as is mplx_reserve_positions.
 *
 * Errors: MPLX_ERR_ARG for NULL required pointers, what include/mplx_conflict.h says of a mplx_conflict_in (step,
 * n_steps, mode) and include/mplx_traj.h of a set, a table over MPLX_RESERVE_MAX_BYTES, Q < 1, a query whose t0 or
 * radius is negative or not finite, a `tab` of another context or with a number of queries other than Q (no tab: Q must
 * be 1), n_nodes < 0, lists without count / action / cost, node_stride < 1, more than 2^31 - 2 list entries,
 * parent_stride < n_nodes; MPLX_ERR_STATE for a poly without a solve or load, chains without params / controls, a check
 * before a fill or before mplx_reserve_set_queries, and a positions call before a fill.  A fill with K == 0 leaves an
 * empty table (every later check blocks nothing but the horizon); n_nodes == 0 is a no-op.
 *
 * Park-safe goals.  The check looks at an edge during [tp, tc] only; a robot that has arrived stays where it is, and
 *   the goal bit of an open set (include/mplx_open.h) is a test of geometry.  mplx_reserve_park_device, called right
 *   after mplx_open_push_device on the same frontier, takes the goal bit from the nodes that cannot stay: it walks rows
 *   r < min(*d_rows->count, n_max, d_rows->capacity).  A row IS LOOKED AT iff its id is in [0, n_nodes) of the open
 *   set's table and flags[id] has MPLX_OPEN_IS_GOAL; on a table with several queries also: its query in [0, Q) (else
 *   q = 0).  For such a row, t_node = the row's t (state row 4D+1) and pos = its state rows 0 .. D-1:
 *   Instants.  Every i in [0, n_steps) with tl_i = (double)i * step - t0[q] >= t_node.  Closed at t_node.  A node past the
 *              horizon (or with a t that is NaN) has no instants and is not vetoed.  (The kernel finds the first instant
 *              from a guess and a scan of at most 4 instants; the set is the one stated.)
 *   Pair test. The check's: against every b that is included, active at i and has group[b] != ignore[q], d2 (dx = pos -
 *              pos_b) and rr = radius[q] + radius[b]; a conflict iff d2 < rr * rr.  Strict; a NaN is no conflict.
 *   Result.    On any conflict the node is VETOED: flags[id] &= ~MPLX_OPEN_IS_GOAL.  Nothing else of the open set
 *              changes: the node stays open (or closed) with its key and is expanded like any other -- with wait edges
 *              (include/mplx_wait.h) and time keys the same lattice state can be reached later.  hit[r] (optional,
 *              [capacity of d_rows] int64) = the minimum of ((int64)i << 32 | b) over the row's conflicts, -1 for a row
 *              without one and for a walked row that is not looked at; rows that are not walked are not written.
 *              *n_vetoed (optional, one int64) grows by the rows vetoed.  A frontier holds every id once.
 *   All outputs are minima and integer sums: pure functions of the inputs.  Asynchronous on the context's stream, no
 *   host read.  Errors as the check's (NULL res / open / frontier, n_max < 0, a frontier without id / state / count or
 *   with state_stride < capacity, an open set of another context or whose table has a number of queries other than Q:
 *   MPLX_ERR_ARG; before a fill or mplx_reserve_set_queries, or on a table with a status bit: MPLX_ERR_STATE).
 *   n_max == 0 and a frontier of capacity 0 are no-ops.  Protection holds to the table's horizon only. */
#ifndef MPLX_RESERVE_H
#define MPLX_RESERVE_H

#include "mplx_conflict.h"
#include "mplx_open.h"
#include "mplx_solve.h"
#include "mplx_table.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mplx_reserve mplx_reserve;

enum { MPLX_RESERVE_MAX_BYTES = 1 << 30 };

int mplx_reserve_create(mplx_ctx *ctx, mplx_reserve **out);
/* Destroy it before its context.                                                                                     */
void mplx_reserve_destroy(mplx_reserve *res);

/* The set of `poly` (of the same context) / K action chains; d_in / h_in as mplx_poly_conflicts / mplx_traj_conflicts
 * take it.                                                                                                            */
int mplx_reserve_fill_poly_device(mplx_reserve *res, mplx_poly *poly, const mplx_conflict_in *d_in);
int mplx_reserve_fill_poly(mplx_reserve *res, mplx_poly *poly, const mplx_conflict_in *h_in);
int mplx_reserve_fill_traj_device(mplx_reserve *res, mplx_ctx *ctx, const mplx_traj_set *d_set, const mplx_conflict_in *d_in);
int mplx_reserve_fill_traj(mplx_reserve *res, mplx_ctx *ctx, const mplx_traj_set *h_set, const mplx_conflict_in *h_in);
/* B, n_steps, step of the last fill (any pointer may be NULL).                                                       */
int mplx_reserve_shape(mplx_reserve *res, int64_t *n_traj, int32_t *n_steps, double *step);
/* Downloads the table, for tests: h_pos [n_steps][D][B], h_active [n_steps][B], h_included [B], h_radius [B], h_group
 * [B], h_status [B]; any may be NULL.  Synchronises.                                                                 */
int mplx_reserve_positions(mplx_reserve *res, double *h_pos, uint8_t *h_active, uint8_t *h_included, double *h_radius,
                           int32_t *h_group, uint8_t *h_status);

/* Host pointers, [Q] each; h_ignore_group_or_null == NULL: -1 each.                                                  */
int mplx_reserve_set_queries(mplx_reserve *res, int32_t Q, const double *h_t0, const double *h_radius,
                             const int32_t *h_ignore_group_or_null);

int mplx_reserve_check_device(mplx_reserve *res, mplx_table *tab_or_null, const mplx_succ_lists *d_lists, int64_t n_nodes,
                              const int32_t *d_parent_id, const double *d_parent_state, int64_t parent_stride,
                              int64_t *d_hit_or_null, int64_t *d_n_blocked_or_null);

/* d_rows: the frontier that was just pushed into `open`; d_hit_or_null: [capacity of d_rows].                        */
int mplx_reserve_park_device(mplx_reserve *res, mplx_open *open, const mplx_table_frontier *d_rows, int64_t n_max,
                             int64_t *d_hit_or_null, int64_t *d_n_vetoed_or_null);

#ifdef __cplusplus
}
#endif
#endif
