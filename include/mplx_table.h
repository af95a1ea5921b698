/* mplx_table.h -- a persistent node table on the device: the search state of a label-correcting sweep (the nodes of
 * StateSpace::hm_, their g values and best back-pointers), the relaxation of whole batches of successor lists against
 * it, and the next frontier.  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * A table holds up to node_capacity nodes, numbered densely from 0 in creation order.  A node has
 *   hash         the 64-bit lattice hash; as in the reference a node's identity IS this hash (waypoint.h:128-135)
 *   state        4D+2 doubles: the successor state that created the node, never rewritten (State::coord)
 *   g            cost-to-come, +inf until a candidate lowers it
 *   pred         node id of the best parent, -1 for a seed (only the best predecessor is kept: no LPA*)
 *   pred_action  the control index that leads from pred to the node (-1 for a seed)
 *
 * mplx_table_relax_device takes the lists of mplx_expand_lists_device (count, action, cost, hash, state), one row per
 * expanded node, plus parent_id[n_nodes], parent_g[n_nodes] and g_max.  List entry e = k*S + j COUNTS iff
 *   j < count[k],  parent_id[k] >= 0,  cost[e] is finite (graph_search.h:81 skips blocked successors), and
 *   cand = parent_g[k] + cost[e] (one IEEE add, graph_search.h:107) is finite, >= 0 and <= g_max.
 * Entries that do not count touch nothing; entries past count[k] are never read.  The result is what the sequential
 * loop of graph_search.h:79-143 produces when it walks the counting entries in ascending e with the parents' g taken
 * from parent_g (a snapshot: the call never reads a parent's g from the table):
 *   1. every hash not in the table becomes a node; ids ascend with the smallest counting e that carries the hash; the
 *      node takes state = column e of the lists, g = +inf, pred = pred_action = -1;
 *   2. for every node, m = the minimum cand over its counting entries; if m < g (strictly): g = m and (pred,
 *      pred_action) = (parent_id[k], action[e]) of the SMALLEST e with cand == m; otherwise the node is unchanged;
 *   3. the next frontier = the nodes improved in this call, each once, ordered by that winning e: id, the new g and
 *      the state rows gathered from the table, laid out so that the next round passes them as d_nodes / node_stride of
 *      mplx_expand_lists_device and as parent_id / parent_g of the next relax.
 * Every output is a pure function of the inputs (no result depends on which thread wins a race).  A cand of -0.0 is
 * stored as +0.0.
 *
 * mplx_table_seed hashes states with the context's control flag (the expansion kernels' device function) and runs the
 * same create-and-improve rule with pred = -1, the seed order as e and cand = the given g (default 0).
 *
 * Capacity: the node arrays full, a probe sequence as long as the hash table (every slot holds another key; as the
 * table has more slots than node_capacity, NODES_FULL is raised with it), or a frontier smaller than the improved set
 * raise a sticky status bit.  No call writes outside any array or loops without bound.  After a bit is set the
 * table's contents (and that call's frontier) are unspecified until mplx_table_clear; calls made after the host has
 * seen the bit (mplx_table_stats, or a call with h_count) return MPLX_ERR_STATE, calls queued before that do nothing.
 * node_capacity >= nodes before the call + counting entries always suffices, and so does a frontier of n_nodes*S.
 *
 * A table belongs to its context (stream, scratch, staging arena): destroy it before the context.  The lists must be
 * final: a relax behind an expansion with yaw controls first lets the context check that launch's heading-limit
 * decisions (which synchronises when any is pending).
 *
 * Errors: MPLX_ERR_ARG for NULL required pointers, n_nodes < 0, lists without hash / cost / action / state, strides
 * smaller than counts, more than 2^31 - 2 list entries, node_capacity < 1 or >= 2^31, 2^slots_log2 <= node_capacity;
 * MPLX_ERR_STATE for a seed without params / controls and for a table with a status bit.  n_nodes == 0 is a successful
 * no-op with frontier count 0.
 *
 * A table can also hold the nodes of several queries at once, a node then being a (query, hash) pair: that form, what
 * it changes for relax, and which of the calls below it refuses are in include/mplx_multi.h.  Planning again on the
 * same table after the robot has moved or the map was edited -- which nodes are kept, with their g -- is
 * include/mplx_replan.h.
 *
 * Time keys.  Among moving obstacles (include/mplx_reserve.h) one lattice state at two times is two nodes.  The
 * reference has the switch, Waypoint::enable_t (waypoint.h:119-122): the time is the last hash_combine.  After
 * mplx_table_set_time_keys(tab, 1) the KEY of a list entry or a seed is combine(hash, (int)std::round(t / 0.1)), with
 * combine the classic boost::hash_combine the lattice hash is built from, hash the entry's hash row (a seed's: the
 * hash of its state) and t the entry's own t row (field 4D+1 of its state column).  Every rule above and in
 * include/mplx_multi.h then reads "key" for "hash": identity, creation order, the per-query regions.  The hash column
 * of the view holds the key, mplx_table_find / _find_multi compare keys (mplx_time_key folds on the host), and the
 * "same lattice state as the goal" test of an open set, which compares that column with the goal's hash, no longer
 * fires.  The switch applies to an empty table only -- after create or clear, before the first seed or relax with
 * entries; otherwise MPLX_ERR_STATE -- and survives mplx_table_clear.  With it off a table runs the launches and
 * produces the bytes it always did; with it on a seed and a relax make one more launch, which writes the keys of the
 * entries within their count into the table's scratch.  mplx_table_rebase_* on such a table: MPLX_ERR_STATE.       */
#ifndef MPLX_TABLE_H
#define MPLX_TABLE_H

#include "mplx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mplx_table mplx_table;

enum { MPLX_TABLE_NODES_FULL = 1, MPLX_TABLE_PROBE_FULL = 2, MPLX_TABLE_FRONTIER_FULL = 4 };

/* Device pointers owned by the table; rows [0, n_nodes) are valid.  state is field-major [4D+2][state_stride].      */
typedef struct {
  const uint64_t *hash;
  const double *g;
  const int32_t *pred;
  const int32_t *pred_action;
  const double *state;
  int64_t state_stride;
} mplx_table_view;

/* A frontier: caller-owned device pointers.  id / g: [capacity]; state: field-major [4D+2][state_stride],
 * state_stride >= capacity; count: one int64, written by every seed / relax call.                                   */
typedef struct {
  int32_t *id;
  double *g;
  double *state;
  int64_t state_stride, capacity;
  int64_t *count;
} mplx_table_frontier;

/* slots_log2 = 0: the hash table gets the smallest power of two >= 2 * node_capacity slots; otherwise 2^slots_log2
 * (> node_capacity, slots_log2 <= 31) -- a knob for tests that want long probe chains.                              */
int mplx_table_create(mplx_ctx *ctx, int64_t node_capacity, int32_t slots_log2, mplx_table **out);
void mplx_table_destroy(mplx_table *tab);
/* Empties the table and its status; asynchronous on the context's stream.                                           */
int mplx_table_clear(mplx_table *tab);
/* Time keys on (on != 0) or off; an empty table only (see above).                                                   */
int mplx_table_set_time_keys(mplx_table *tab, int32_t on);
/* combine(hash, (int)std::round(t / 0.1)) on the host: the key of (hash, t) in a table with time keys.              */
uint64_t mplx_time_key(uint64_t hash, double t);
int mplx_table_view_of(mplx_table *tab, mplx_table_view *view);
/* Number of nodes and the status bits; synchronises.  Either pointer may be NULL.                                   */
int mplx_table_stats(mplx_table *tab, int64_t *n_nodes, uint32_t *status);
/* (the text of a failed call: mplx_last_error of the table's context)                                               */

/* h_states: field-major [4D+2][stride], n <= stride; h_g_or_null: [n].  Host pointers, staged through the context's
 * arena; synchronises on return.  h_count_or_null receives the frontier count.                                      */
int mplx_table_seed(mplx_table *tab, const double *h_states, int64_t n, int64_t stride, const double *h_g_or_null,
                    const mplx_table_frontier *d_frontier, int64_t *h_count_or_null);
/* Asynchronous on the context's stream.  d_entry_id_or_null ([n_nodes * S]) receives per list entry the node id, or
 * -1 for an entry that does not count (entries past count[k] included).  h_count_or_null != NULL reads the frontier
 * count back, with one synchronisation.                                                                             */
int mplx_table_relax_device(mplx_table *tab, const mplx_succ_lists *d_lists, int64_t n_nodes, const int32_t *d_parent_id,
                            const double *d_parent_g, double g_max, const mplx_table_frontier *d_next,
                            int32_t *d_entry_id_or_null, int64_t *h_count_or_null);
/* id of every hash, -1 for a hash the table does not hold.  The host form synchronises.                             */
int mplx_table_find_device(mplx_table *tab, const uint64_t *d_hash, int64_t n, int32_t *d_id);
int mplx_table_find(mplx_table *tab, const uint64_t *h_hash, int64_t n, int32_t *h_id);
/* Walks pred from `id` back to a seed and returns the chain root first: h_ids[0 .. n_edges] and h_actions[0 ..
 * n_edges), h_actions[i] leading from h_ids[i] to h_ids[i + 1].  h_ids holds cap + 1 entries, h_actions cap.  The
 * walk is bounded by the number of nodes; a chain of more than cap edges returns MPLX_ERR_ARG.  Synchronises.       */
int mplx_table_path(mplx_table *tab, int32_t id, int32_t *h_ids, int32_t *h_actions, int64_t cap, int64_t *n_edges);

#ifdef __cplusplus
}
#endif
#endif
