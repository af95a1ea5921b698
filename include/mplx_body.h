/* mplx_body.h -- attitude-aware body checks: the robot as an axisymmetric ellipsoid whose axis follows the thrust
 * direction acc + g e_z, tested against an obstacle point cloud at samples of successor-list entries and of polynomial
 * trajectories.  A search that calls the list check between its expansion and its relax (include/mplx_table.h) plans
 * for a body instead of a point: a gap the vehicle passes only tilted or only because it is flat stays open, and the
 * acceleration of the ACC and JRK state spaces reaches a collision test.  Exported by libmplx.so next to
 * include/mplx.h, whose ABI version it does not change.  The reference has nothing of the kind (its SE(3) planning
 * lives in an environment this library does not model); what is normative is stated here and restated sequentially in
 * tests/body_model.py.
 *
 * All arithmetic is IEEE double under -ffp-contract=off, in the order written, with + - * / and comparisons only: no
 * sqrt and no trigonometry runs on the device, so host, device and model agree bit for bit.
 *
 * Shape.  mplx_body_set_shape(body, r, h, g, min_cos_tilt): r the radius across the thrust axis, h the half-height
 *   along it (both finite and > 0), g > 0 (finite), min_cos_tilt in [0, 1): the cosine of the largest tilt, computed by
 *   the caller once (the device only multiplies).  Derived once on the host: R = max(r, h), RR = (R * R) * 1.0000001,
 *   and the products r * r, h * h, min_cos_tilt * min_cos_tilt.
 *
 * Cloud.  n points of D doubles each, from host memory (mplx_body_fill), device memory (mplx_body_fill_device,
 *   asynchronous) or the cells of class `kind` of the map the context holds now (mplx_body_fill_map: point p is point p
 *   of mplx_map_cloud(kind); the points never cross the host link, the call reads their number back).  A point with a
 *   coordinate that is not finite is EXCLUDED: it never hits and keeps its index.  n == 0 is an empty cloud that
 *   blocks nothing.  n * D * 8 > MPLX_BODY_MAX_BYTES (1 GiB) or n > 2^31 - 2 is MPLX_ERR_ARG.  A fill replaces the
 *   previous cloud and increases the generation that mplx_body_shape reports; mplx_body_set_shape after a fill keeps
 *   the points (and the generation) and bins them again.
 *
 * The pair test.  Inputs: a body centre c[D], an acceleration a[D], a point p[D].  In 2-D d_z = 0 and a_z = 0: one
 *   formula serves both dimensions, in 2-D it is the section of the tilted ellipsoid by the plane.
 *   Attitude.   n = (a_x, a_y, a_z + g);  nn = (n_x*n_x + n_y*n_y) + n_z*n_z.
 *               The sample has a BAD ATTITUDE iff  !(n_z > 0) || n_z*n_z < (min_cos_tilt*min_cos_tilt) * nn :
 *               thrust pointing down or vanishing, tilt beyond the limit, a NaN in n_z.  Such a sample makes no point
 *               test.  (A NaN in n_x or n_y alone fails neither comparison; every point test of the sample is then false.)
 *   Point test. d = p - c;  dd = (d_x*d_x + d_y*d_y) + d_z*d_z;  dn = (d_x*n_x + d_y*n_y) + d_z*n_z;
 *               a2 = dn*dn / nn;  perp2 = dd - a2;  e = perp2 / (r*r) + a2 / (h*h).
 *               p is INSIDE iff  dd <= RR && e <= 1.0.  Closed: a point on the surface is inside.  A NaN is not.
 *   The conjunct dd <= RR never changes the mathematical outcome (e <= 1 implies dd <= R^2 up to a few ulp, far inside
 *   the slack of RR); it makes the definition independent of any spatial pruning.
 *
 * List check.  mplx_body_check_device looks at the lists of mplx_expand_lists_device (count, action, cost), one row per
 *   expanded node, with parent_id[n_nodes] and the parents' state rows (field-major [4D+2][parent_stride]), as
 *   mplx_reserve_check_device takes them (include/mplx_reserve.h).  Entry e = k * S + j IS LOOKED AT iff
 *     j < count[k],  parent_id[k] >= 0,  cost[e] is finite,  action[e] in [0, nU).
 *   Wait entries (include/mplx_wait.h) are entries like any other.
 *   Samples.  i = 0 .. n_samp (n_samp >= 1): s_i = (double)i * (dt / (double)n_samp) for i < n_samp, s_{n_samp} = dt.
 *   Centre and acceleration at s_i: the position and the acceleration mplx_traj_sample gives in Command form for a
 *     chain through this edge -- traj::eval_segment on the segment traj::chain_segment builds from (parent state,
 *     U[action[e]]).  Yaw does not enter: the body is axisymmetric.
 *   Key.      A bad attitude at sample i: ((int64)i << 32) | 0x7fffffff.  A point p inside at sample i:
 *             ((int64)i << 32) | p.  hit[e] (optional, [n_nodes * S] int64) = the minimum key, -1 for an entry
 *             without one and for every entry j < S of the n_nodes rows that is not looked at.
 *   Result.   An entry with a key is BLOCKED: cost[e] = +inf.  No other byte of the lists changes.  *n_blocked
 *             (optional, one int64) is increased by the number of entries blocked in this call.
 *   Every output is a minimum or a sum of integers: a pure function of the inputs whatever the tiling and whatever the
 *   cell edge of the cloud's grid.
 *   Like the reservation check it first lets the context finalise the pending heading-limit decisions of an expansion
 *   with yaw controls, then runs asynchronously on the context's stream with no host read.
 *
 * Trajectory-set check.  mplx_body_check_poly_device looks at the K problems of `poly` (its last solve or load).
 *   in->step > 0 and finite.  Problem k is EXCLUDED, with hit = -1, under the set's status rules of
 *   include/mplx_reserve_poly.h (any status bit, S == 0).  Otherwise, with total_k the problem's total time (the scaled
 *   total where it holds a Lambda, include/mplx_scale.h):
 *   Samples.  tl_i = (double)i * step for every i >= 0 with tl_i <= total_k, plus one last sample at total_k itself,
 *             whose index is one past the largest such i; it is made even when it equals the previous sample.
 *             (Indices stop at 2^31 - 2: a step that small against the total is the caller's error.)
 *   Centre and acceleration: bit for bit what mplx_poly_sample gives in Command form at those times; a Lambda is
 *             honoured exactly as that call honours it.
 *   Keys and hit[k] as above; status[k] = the set's status bits of problem k; *n_hit is increased by the problems with
 *   hit != -1.  Every pointer of the out struct is optional.  The host-pointer twin copies its [K] rows through a row
 *   buffer that the body owns (not the context's staging arena) and is synchronous.
 *
 * Errors.  MPLX_ERR_ARG: NULL required pointers, r / h / g / min_cos_tilt outside what is stated, n < 0 or over the
 *   limits, n_samp < 1, a step that is not > 0 and finite, a poly of another context, n_nodes < 0, lists without count /
 *   action / cost, node_stride < 1, more than 2^31 - 2 list entries, parent_stride < n_nodes.  MPLX_ERR_STATE: a check
 *   before mplx_body_set_shape or before any fill, mplx_body_fill_map without a map, a poly without a solve or load,
 *   lists without params / controls, mplx_body_cells before a fill and a shape.  n_nodes == 0 and K == 0 are no-ops.
 *   Failures are statuses, never faults.
 *
 * The grid (not normative: no result depends on it).  The included points are binned into a uniform grid over their
 *   bounding box, cell edge a hair above sqrt(RR), doubled until the box needs at most 2^22 cells; a sample visits the
 *   3^D cells around its centre.  MPLX_BODY_CELL_MULT (an integer >= 1, read at mplx_body_create) multiplies the
 *   automatic edge, so that a test can show the bytes do not depend on it.  mplx_body_shape and mplx_body_cells hand
 *   the binning out, for tests; both synchronise. */
#ifndef MPLX_BODY_H
#define MPLX_BODY_H

#include "mplx_solve.h"
#include "mplx_table.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mplx_body mplx_body;

enum { MPLX_BODY_MAX_BYTES = 1 << 30 };
enum { MPLX_BODY_BAD_ATTITUDE = 0x7fffffff }; /* the low word of a key that reports a bad attitude */

int mplx_body_create(mplx_ctx *ctx, mplx_body **out);
/* Destroy it before its context.                                                                                     */
void mplx_body_destroy(mplx_body *body);

int mplx_body_set_shape(mplx_body *body, double r, double h, double g, double min_cos_tilt);

/* [n][D] doubles.  The host form is synchronous.                                                                     */
int mplx_body_fill(mplx_body *body, const double *h_xyz, int64_t n);
int mplx_body_fill_device(mplx_body *body, const double *d_xyz, int64_t n);
/* kind: MPLX_CELL_OCCUPIED / _FREE / _UNKNOWN of include/mplx_map_util.h.                                            */
int mplx_body_fill_map(mplx_body *body, int kind);

/* Any pointer may be NULL.  n, n_excluded, the generation; after a shape and a fill also the grid: cells per axis
 * ([3], 1 for the axes past D), the cell edge and the origin ([3]); without them cells = 0 and edge = 0.  Synchronises. */
int mplx_body_shape(mplx_body *body, int64_t *n, int64_t *n_excluded, int32_t *cells_per_axis, double *cell_edge,
                    double *origin, int64_t *generation);
/* h_cell_of_point [n] (-1: excluded), h_cell_start [cells + 1] (cell c holds cell_start[c + 1] - cell_start[c] points);
 * either may be NULL.  Synchronises.                                                                                 */
int mplx_body_cells(mplx_body *body, int32_t *h_cell_of_point, int32_t *h_cell_start);

int mplx_body_check_device(mplx_body *body, const mplx_succ_lists *d_lists, int64_t n_nodes, const int32_t *d_parent_id,
                           const double *d_parent_state, int64_t parent_stride, int32_t n_samp, int64_t *d_hit_or_null,
                           int64_t *d_n_blocked_or_null);

typedef struct {
  double step; /* > 0, finite */
} mplx_body_poly_in;

typedef struct {
  int64_t *hit;    /* [K] the minimum key, -1 none                         */
  uint8_t *status; /* [K] the set's status bits                            */
  int64_t *n_hit;  /* one counter, increased by the problems with hit != -1 */
} mplx_body_poly_out; /* every pointer optional */

/* in: a host struct in both forms; out: device pointers / host pointers.                                             */
int mplx_body_check_poly_device(mplx_body *body, mplx_poly *poly, const mplx_body_poly_in *in, const mplx_body_poly_out *d_out);
int mplx_body_check_poly(mplx_body *body, mplx_poly *poly, const mplx_body_poly_in *in, const mplx_body_poly_out *h_out);

#ifdef __cplusplus
}
#endif
#endif
