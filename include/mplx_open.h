/* mplx_open.h -- the open set of a node table (include/mplx_table.h): a priority per node, which nodes are open, which
 * lie in the goal region, the selection of the next batch to expand and the rule that says when the goal is proven.
 * With mplx_table_relax_device it makes a goal-directed search that stays on the device but for one small result per
 * round.  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * An open set belongs to one table and has, per node id of that table,
 *   f      the key the node was pushed with last
 *   flags  MPLX_OPEN_SEEN (pushed at least once), MPLX_OPEN_IS_OPEN, MPLX_OPEN_IS_GOAL (inside the goal region)
 * Both are zero / unspecified for a node that was never pushed.  The semantics are those of the sequential rule below.
 *
 * mplx_open_push_device walks rows r = 0 .. min(*d_rows->count, n_max, d_rows->capacity) - 1 of a frontier that
 * mplx_table_seed / mplx_table_relax_device wrote (the count is read on the device: no host read-back, the relax in
 * front of the push stays asynchronous).  A row whose id is not in [0, n_nodes) of the table is ignored.  Otherwise
 *   h, tol  the default heuristic (env_base.h:46-64) and the goal tolerance test (env_map.h:25-37) of the row's state,
 *           the table's hash[id] and the context's goal (mplx_set_goal), as the heur / flags rows of the lists state them
 *   f       = g_row + eps * h: one multiply and one add, never contracted; for eps == 0, f = g_row
 *           (graph_search.h:53, :88, :119).  A row whose f is not >= 0 (a NaN, a negative g) is ignored.
 *   f[id]   = f;   flags[id] = SEEN | IS_OPEN | (goal ? IS_GOAL : 0)
 * where goal = tol, and with sight != 0 additionally: the ray of env_map.h:38-43 from the row's position to the goal
 * meets no occupied cell (the rule and the device code of mplx_goal_sight_device, include/mplx_ray.h).  A pushed node
 * that was closed is open again (re-opening, graph_search.h:135-141); an open node's key is replaced.  A frontier holds
 * every id once; rows with equal ids and different values leave that node's f and flags unspecified.
 *
 * mplx_open_select_device: let O = the nodes with IS_OPEN and G = the nodes with IS_GOAL, open or closed.
 *   f_min   = min f over O, +inf when O is empty
 *   goal_f  = min f over G;  goal_id = the smallest id in G with f == goal_f;  goal_g = the table's g[goal_id]
 *             (G empty: goal_id = -1, goal_f = goal_g = +inf)
 *   status  MPLX_OPEN_FOUND     if G is not empty and goal_f <= f_min: nothing is selected, count = 0.  (A*'s "the goal
 *                               is at the top of the heap" for batches: a goal node popped early inside a wide batch is
 *                               announced only once no open key is below it.)
 *           MPLX_OPEN_EMPTY     otherwise, if O is empty: count = 0
 *           MPLX_OPEN_SELECTED  otherwise: T = f_min + delta (one add; +inf allowed); the selected set is the open
 *                               nodes with f <= T in ascending id.  If more than d_out->capacity are selected only the
 *                               first that many by id are taken and the rest stay open: no error, no status bit.
 *   The selected nodes lose IS_OPEN and go to d_out as id, the table's current g[id] and the state rows gathered from
 *   the table -- the layout mplx_table_relax_device emits, so d_out is the next expansion's d_nodes / node_stride and the
 *   next relax's parent_id / parent_g.  *d_out->count = result.count = their number; n_open = the nodes still open
 *   after the call.  Every output is a pure function of the inputs (no result depends on which thread wins a race).
 * h_result_or_null != NULL reads the result (48 bytes) back with one synchronisation: a search round's only read-back.
 *
 * The arrays are sized by the table's node_capacity when the open set is created.  mplx_open_clear empties the set
 * (asynchronous); call it whenever the table is cleared.  Destroy the open set before its table.
 *
 * Errors: MPLX_ERR_ARG for NULL required pointers, n_max < 0, delta < 0 or NaN, eps negative, NaN or infinite, and a
 * frontier without id / g / state / count or with state_stride < capacity or capacity < 0; MPLX_ERR_STATE for a table
 * with a status bit (calls queued before the host saw the bit do nothing), for a push without a goal, and for a push
 * with sight != 0 without a map.  n_max == 0, a frontier of capacity 0 and a table without nodes are successful
 * no-ops of push; a select then returns MPLX_OPEN_EMPTY.  No call writes past the capacity of any array or loops
 * without bound.
 *
 * The open set of a table with several queries has one goal and one result per query: include/mplx_multi.h.  The push
 * that sets keys and goal bits without opening the nodes (after a rebase of the table): include/mplx_replan.h.  The
 * heuristic that follows a prior trajectory per query: include/mplx_prior.h.                                         */
#ifndef MPLX_OPEN_H
#define MPLX_OPEN_H

#include "mplx_table.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mplx_open mplx_open;

enum { MPLX_OPEN_IS_OPEN = 1, MPLX_OPEN_IS_GOAL = 2, MPLX_OPEN_SEEN = 4 };  /* per-node flags byte */
enum { MPLX_OPEN_SELECTED = 0, MPLX_OPEN_FOUND = 1, MPLX_OPEN_EMPTY = 2 };  /* result.status       */

/* Device pointers owned by the open set, [node_capacity of the table] each; entries [0, n_nodes) are meaningful.    */
typedef struct {
  const double *f;
  const uint8_t *flags;
} mplx_open_view;

typedef struct {
  int32_t status, goal_id;
  int64_t count, n_open;
  double f_min, goal_f, goal_g;
} mplx_open_result;

int mplx_open_create(mplx_table *tab, mplx_open **out);
void mplx_open_destroy(mplx_open *o);
/* Asynchronous on the context's stream.                                                                             */
int mplx_open_clear(mplx_open *o);
int mplx_open_view_of(mplx_open *o, mplx_open_view *v);
/* Asynchronous.  d_rows: a frontier in device memory (its count included).                                          */
int mplx_open_push_device(mplx_open *o, const mplx_table_frontier *d_rows, int64_t n_max, double eps, int32_t sight);
/* d_out: the frontier that receives the selection.  d_result_or_null: device memory for the result.                 */
int mplx_open_select_device(mplx_open *o, double delta, const mplx_table_frontier *d_out,
                            mplx_open_result *d_result_or_null, mplx_open_result *h_result_or_null);

#ifdef __cplusplus
}
#endif
#endif
