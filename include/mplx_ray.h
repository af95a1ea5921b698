/* mplx_ray.h -- MapUtil<Dim>::rayTrace on the device, and the line-of-sight half of env_map::is_goal.
 * Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * One ray takes p1, p2 (D doubles each) on the map the context holds NOW: mdim, origin, res and the int8 cells of
 * mplx_set_map as edited since (mplx_edit_map, mplx_map_dilate, ...) -- not the potential copy and not the blocked
 * bits, which fold in the search region.  Bit for bit the reference's arithmetic (map_util.h:117-134, :103-108; no
 * contraction):
 *
 *   diff_i   = p2_i - p1_i
 *   linf     = max_i |diff_i / res|
 *   max_diff = (int)(linf / 0.8)                          truncation
 *   s        = 1.0 / max_diff;  step_i = diff_i * s
 *   for n = 1 .. max_diff - 1:
 *     pt_i = p1_i + step_i * (double)n                    one multiply, one add
 *     c_i  = round((pt_i - origin_i) / res - 0.5)         floatToInt
 *     c outside the map: stop, MPLX_RAY_LEFT_MAP
 *     c != the cell of step n - 1: emit c                 consecutive duplicates only
 *
 * max_diff <= 1 emits nothing; neither p1's cell (step 0) nor p2's (step max_diff) is visited.  An occupied cell
 * (== 100; 37, 101, 127, -5, -1 are not occupied, map_util.h:48) does NOT stop the trace: rayTrace returns the whole
 * list and is_goal (env_map.h:38-43) then looks for an occupied cell in it -- here MPLX_RAY_HIT and first_hit.
 *
 * Where the reference converts an unrepresentable double to int (undefined behaviour) the engine defines the result:
 * a ray with a non-finite coordinate or with linf / 0.8 >= 2^31 is MPLX_RAY_BAD (nothing traced, n_cells 0), and a
 * step whose round(...) is not in [0, mdim_i) when compared AS A DOUBLE is outside (NaN and huge values included).
 *
 * Errors: MPLX_ERR_STATE without a map (mplx_goal_sight_device: or without a goal from either source); MPLX_ERR_ARG
 * for n < 0, stride < n, a NULL status, NULL points with n > 0, lanes not in {0, 4, 16, 64}, cell_cap < 0, cells with
 * cell_cap == 0, lists without count or state, NULL d_flags.  n == 0 is a successful no-op.                        */
#ifndef MPLX_RAY_H
#define MPLX_RAY_H

#include "mplx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_RAY_LEFT_MAP = 1, MPLX_RAY_HIT = 2, MPLX_RAY_BAD = 4, MPLX_RAY_TRUNCATED = 8 };
enum { MPLX_FLAG_GOAL_BLOCKED = 8 }; /* bit 3 of the flags row of mplx_succ_lists / mplx_post            */

typedef struct {
  uint8_t *status;      /* [n] bits above; required                                              */
  int32_t *n_cells;     /* [n] rayTrace(p1,p2).size(), or NULL                                   */
  int32_t *first_hit;   /* [n] getIndex of the first occupied cell in emission order, -1; or NULL */
  int32_t *cells;       /* [n][cell_cap] getIndex of the emitted cells in order, or NULL         */
  int32_t cell_cap;     /* first min(n_cells, cell_cap) entries of a row are written, the rest untouched;
                           TRUNCATED when n_cells > cell_cap and cells != NULL                    */
} mplx_ray_out;

/* Points are field-major [D][stride] like node rows; p2_stride == 0: one p2 (D consecutive doubles) for all rays.
 * lanes: 0 (automatic) or 4 / 16 / 64, the lanes of a wavefront that share one ray; results never depend on it.
 * Asynchronous on the context's stream; the caller synchronises (mplx_synchronize) before it reads the outputs.   */
int mplx_ray_trace_device(mplx_ctx *ctx, const double *d_p1, const double *d_p2, int64_t n, int64_t stride,
                          int64_t p2_stride, int32_t lanes, const mplx_ray_out *d_out);
/* The same with host pointers: staged through the context's arena; synchronous.  (lanes == 0 here goes by the
 * longest ray of the call, the device-pointer call by the map's longest axis.)                                    */
int mplx_ray_trace(mplx_ctx *ctx, const double *h_p1, const double *h_p2, int64_t n, int64_t stride,
                   int64_t p2_stride, int32_t lanes, const mplx_ray_out *h_out);

/* The ray trace of env_map::is_goal (env_map.h:38-43) for lists that stay on the device.  For every emitted
 * successor (j < count[k]) whose d_flags[k*S + j] has bit 0 set (inside the goal tolerances), the ray from the
 * successor's position (state rows 0 .. D-1) to the goal position is traced, and MPLX_FLAG_GOAL_BLOCKED is ORed into
 * the entry when an emitted cell is occupied: afterwards (flags & 9) == 1 is the reference's is_goal.  Every other
 * bit and every other byte of d_flags keeps its value.  The goal position is goal_or_null->goal when given, else
 * the one of mplx_set_goal.  d_flags: the row the expansion launch (mplx_succ_lists::flags) or
 * mplx_post_lists_device wrote.  Asynchronous; the candidates are counted and traced without a host read.         */
int mplx_goal_sight_device(mplx_ctx *ctx, const mplx_succ_lists *d_lists, int64_t n_nodes,
                           const mplx_goal_spec *goal_or_null, uint8_t *d_flags);

#ifdef __cplusplus
}
#endif
#endif
