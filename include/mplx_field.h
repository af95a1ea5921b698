/* mplx_field.h -- goal distance fields: the grid distance of every map cell to a goal region, computed on the device by a
 * backward wavefront over the context's blocked-bit map, and the push of an open set (include/mplx_open.h) that takes
 * its heuristic from one.  The reference has nothing of the kind: this header is normative, and tests/field_model.py
 * restates it sequentially.  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * 1. Cells.  The cell of a position is MapUtil::floatToInt per axis, cell = (int)round((pos - origin) / res - 0.5), the
 * arithmetic a sample's look-up uses; the index of a cell is getIndex (x fastest).  A cell is TRAVERSABLE iff a sample in
 * it does not end a primitive: it is inside the map, inside the search region if one is set, and
 *   without a potential map  not occupied: its bit in the context's blocked-bit map is clear.  The field reads those
 *                            bits, the ones the expansion reads; it does not restate the rule
 *   with a potential map     the potential value is < 100 (env_map.h:113-118; the occupancy is not consulted).  Values
 *                            1 .. 99 COST, they do not block.  The context's bits are a pre-screen there -- set for
 *                            every cell with a value > 0 -- and a field over them would take a cost cell for a wall and
 *                            overestimate; so the build derives bits of its own from the potential map and the region
 *
 * 2. The field.  For f < F, dist[f][c] is an int32, stored [F][n_cells].  The seeds of field f are the cells of the
 * inclusive box lo[f][D] .. hi[f][D] (cell indices), clipped to the map; a box that clips to nothing has no seed.
 *   dist[f][c] = 0    on every seed cell, traversable or not
 *              = the length in steps of the shortest chain of cells from c to a seed cell of f, where consecutive cells
 *                differ by at most 1 on every axis (8 neighbours in 2-D, 26 in 3-D) and every cell of the chain is
 *                traversable except the seed it ends in, which need not be.  A diagonal step needs only a traversable
 *                target: there is no corner rule, because the sampled collision check has none
 *              = -1   where no chain exists, and on every non-seed cell that is not traversable
 * This is the unique fixed point of d[c] = min(d[c], 1 + min over the neighbours) on traversable cells, so it is a pure
 * function of the inputs whatever the tiling and the order of work.  The number of passes a build took is not, and is
 * part of no result.
 *
 * 3. Calls.  mplx_field_build takes host arrays [F][D]; it builds the blocked bits if they are not current, runs the
 * passes and returns when the field is complete (it reads one 8-byte counter back per pass).  F == 0 leaves an empty
 * field.  mplx_field_download is synchronous and for tests.  A field is STALE once anything that can change a blocked
 * bit has run on its context since the build: mplx_set_map, mplx_edit_map, mplx_set_potential,
 * mplx_update_potential_map, mplx_set_region, mplx_set_search_region_path, the MapUtil calls that rewrite the map and a
 * broadcast map.  mplx_field_is_stale answers 1 / 0 (MPLX_ERR_ARG for NULL).  Destroy a field before its context.  A field
 * destroyed while it is in force in an open set is not read again: every push of that open set is MPLX_ERR_STATE until
 * mplx_open_clear_field, another mplx_open_set_field or mplx_open_set_goals.
 * Errors: MPLX_ERR_ARG for NULL required pointers, F < 0 and F * n_cells * 4 > MPLX_FIELD_MAX_BYTES; MPLX_ERR_STATE
 * without a map, and for a build that did not reach its fixed point within n_cells + 1 passes (which cannot happen: after
 * pass p every cell whose shortest chain crosses at most p tile borders is final, and a chain has fewer than n_cells
 * steps).  No call writes past an array or loops without a bound.
 *
 * 4. The push.  mplx_open_set_field(o, fld, h_field_of_query): [Q] entries, NULL = query q uses field q, -1 = that query
 * keeps the default heuristic.  The field is in force until mplx_open_clear_field, or until mplx_open_set_goals, which
 * drops it for the reason it drops priors (a new goal: the old field does not lead to it).  mplx_open_clear leaves it in
 * force.  Every push (mplx_open_push_device, mplx_open_push_closed_device, with or without sight) of a row of query q
 * with fq = field_of_query[q] >= 0 whose hash is not the goal hash:
 *   c = cell of the row's pos;  n = (c inside the map) ? dist[fq][c] : -1
 *   n < 0:  h = +inf                      (the row is pushed as any row with an infinite key is)
 *   else    L = Linf(pos - goal.pos)      (the expression of the default heuristic)
 *           G = res * (double)max(n - 1, 0)
 *           m = G > L ? G : L
 *           h = w * m / v_max             (the default's expression with m in place of L)
 * Where G <= L the key is bit for bit the default's.  The key rule, the flags and the goal test are untouched.  An open
 * set without a field runs the kernels it ran before this header existed.
 * Errors: MPLX_ERR_STATE for v_max <= 0 (of the goal the pushes use), for a field together with priors -- whichever is
 * set second --, for a push with a stale field, with a field destroyed since, and for an empty field; MPLX_ERR_ARG for a field of another context and
 * for an entry outside [-1, F).
 *
 * 5. Why n - 1, and why h is admissible.  validate_primitive holds every axis speed to v_max.  traverse_primitive samples
 * at most res apart per axis, so consecutive samples of a valid trajectory lie in equal or neighbouring traversable
 * cells (traversable as section 1 has it: every cell a valid primitive can have a sample in, cost cells included).  The end state lies in the goal box, so its cell is a seed, traversable or not.  A path that stays in
 * traversable cells and has Linf length l can be cut into ceil(l / res) pieces whose ends are at most res apart, hence in
 * equal or neighbouring cells: n <= l / res + 1.  The remaining time is therefore at least res (n - 1) / v_max, and
 * effort, potential and yaw costs only add to w times it.  The heuristic is not consistent (a primitive can cross one
 * cell more than v_max dt / res); the open set re-opens, and its stopping rule needs admissibility only.  The seeds must
 * cover the goal region: the caller's box is floatToInt(goal -+ tol) widened by one cell on every side, so that no
 * rounding of goal -+ tol leaves a goal-region cell unseeded; extra seeds only lower dist.                            */
#ifndef MPLX_FIELD_H
#define MPLX_FIELD_H

#include "mplx_open.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MPLX_FIELD_MAX_BYTES (1LL << 30)

typedef struct mplx_field mplx_field;

/* Device pointer owned by the field; NULL / 0 while the field is empty.                                             */
typedef struct {
  const int32_t *dist; /* [F][n_cells] */
  int32_t F;
  int64_t n_cells;
} mplx_field_view;

int mplx_field_create(mplx_ctx *c, mplx_field **out);
void mplx_field_destroy(mplx_field *fld);
int mplx_field_build(mplx_field *fld, int32_t F, const int32_t *h_lo, const int32_t *h_hi);
int mplx_field_shape(mplx_field *fld, int32_t *F, int64_t *n_cells);
int mplx_field_view_of(mplx_field *fld, mplx_field_view *v);
int mplx_field_download(mplx_field *fld, int32_t *h_dist);
int mplx_field_is_stale(mplx_field *fld);
/* diagnostic: passes of the last build (part of no result) */
int mplx_field_passes(mplx_field *fld, int64_t *passes);

int mplx_open_set_field(mplx_open *o, mplx_field *fld, const int32_t *h_field_of_query);
int mplx_open_clear_field(mplx_open *o);

#ifdef __cplusplus
}
#endif
#endif
