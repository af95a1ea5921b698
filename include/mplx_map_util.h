/* mplx_map_util.h -- the MapUtil<Dim> calls a user makes on the map before planning (reference
 * include/mpl_collision/map_util.h), run on the map the context already holds on the device.  Exported by
 * libmplx.so next to include/mplx.h, whose ABI version they do not change.
 *
 * Every call works on the map of mplx_set_map (as edited since: mplx_edit_map, mplx_update_potential_map, the calls
 * below) and never moves it across the host link again: mplx_map_upload_bytes does not change.  A potential map
 * (mplx_set_potential, mplx_update_potential_map) is a separate copy, as env_map's potential_map_ is
 * (env_map.h:181-183), and these calls leave it alone; with one installed the expansion reads only that copy, so
 * its results do not change.  The calls are synchronous: on return the device map holds the result and, where an
 * output pointer is given, the host buffer holds it too.  Cell classes as MapUtil has them (map_util.h:44-48,
 * 308-313): occupied v == 100, free 0 <= v < 100, unknown v == -1; any other value belongs to no class.
 * Errors: MPLX_ERR_STATE when no map is set, MPLX_ERR_ARG for the argument errors named below.                   */
#ifndef MPLX_MAP_UTIL_H
#define MPLX_MAP_UTIL_H

#include "mplx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_CELL_OCCUPIED = 0, MPLX_CELL_FREE = 1, MPLX_CELL_UNKNOWN = 2 };

/* MapUtil::dilate (map_util.h:220-256): every cell that some offset o reaches from a cell occupied in the map as it
 * was before the call (m - o inside the map and occupied) becomes 100; every other cell keeps its value.  offsets:
 * n rows of dim int32 (x, y[, z]); the list may be empty, hold duplicates, the zero offset or offsets larger than the
 * map (no-ops).  MPLX_ERR_ARG for n < 0 or offsets == NULL with n > 0.  h_map_out_or_null: the new map, n_cells
 * bytes in map order.                                                                                              */
int mplx_map_dilate(mplx_ctx *ctx, const int32_t *offsets, int32_t n, int8_t *h_map_out_or_null);
/* MapUtil::freeUnknown (unknown_only = 1: -1 -> 0, nothing else changes) and MapUtil::freeAll (unknown_only = 0:
 * every cell becomes 0), map_util.h:258-296.  MPLX_ERR_ARG for any other unknown_only.                              */
int mplx_map_free(mplx_ctx *ctx, int unknown_only, int8_t *h_map_out_or_null);
/* MapUtil::getCloud / getFreeCloud / getUnknownCloud (map_util.h:136-218), kind MPLX_CELL_*: the cells of that class
 * in the reference's loop order (x outermost, then y, then z innermost), each as intToFloat, ((double)n_i + 0.5) *
 * res + origin_i per axis.  *n_out = the number of cells of the class, always; the first min(*n_out, cap) points
 * are written to xyz_or_null ([cap][dim] doubles; NULL or cap == 0: count only).  MPLX_ERR_ARG for a bad kind,
 * cap < 0 or n_out == NULL.                                                                                       */
int mplx_map_cloud(mplx_ctx *ctx, int kind, double *xyz_or_null, int64_t cap, int64_t *n_out);

#ifdef __cplusplus
}
#endif
#endif
