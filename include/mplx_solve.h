/* mplx_solve.h -- the trajectory solver on the device: K minimum-velocity / acceleration / jerk polynomials through
 * waypoints in one launch, and Trajectory<Dim>'s samples, efforts and env_map::traverse_trajectory on what it returns.
 * Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * Reference: include/mpl_traj_solver/traj_solver.h (TrajSolver::solve, allocate_time), src/mpl_traj_solver/poly_solver.cpp
 * (PolySolver::solve), src/mpl_traj_solver/poly_traj.cpp (setTime, toPrimitives, p()).  Problem k has W_k waypoints and
 * S_k = W_k - 1 segments with durations dts[s].  The ends' control gives the smoothing order so = 0 (VEL), 1 (ACC), 2
 * (JRK): N = 2 (so + 1) coefficients per segment and axis, the integral of the square of derivative so + 1 is minimised,
 * derivatives up to so are continuous at the interior waypoints.  A derivative of a waypoint is FIXED to the waypoint's
 * value when its use bit is set and its order is <= so, otherwise it is free and the minimisation chooses it.
 *
 *   setPath mode (wp_flags == NULL; TrajSolver::setPath): interior waypoints fix their position only, the two ends fix
 *     position .. derivative so -- with the values the waypoint rows hold (the reference's setPath zeroes them; the
 *     Python TrajSolver does the same).
 *   setWaypoints mode: wp_flags[w * flag_stride + k], bits MPLX_USE_POS / _VEL / _ACC, as they are.
 *   dts == NULL: allocate_time, dts[s] = max_i |pos[s+1][i] - pos[s][i]| / v (v_arr[k] when v_arr != NULL).
 *   taus[0] = 0, taus[s+1] = taus[s] + dts[s] by sequential addition; T = taus[S].
 *   yaw: a second, 1-D solve of the waypoints' yaw with yaw_control; only MPLX_VEL is built (y0 = yaw_w, rate =
 *     (yaw_{w+1} - yaw_w) / dts[w]); ACC / JRK yaw is MPLX_ERR_ARG.
 *   The segments become primitives as PolyTraj::toPrimitives makes them: per axis c_j = p_{5-j} (5-j)!, absent ones 0.
 *
 * Bit for bit the reference: dts of allocate_time, taus, the whole so = 0 solve with fixed positions (p0 = pos_w, p1 =
 * (pos_{w+1} - pos_w) / T), the yaw solve, and every sample / effort / traversal of a solved segment given its stored
 * coefficients.  The coefficients for so >= 1 come from a block tridiagonal elimination in waypoint order, not from
 * Eigen's dense LU: equal to rounding (DESIGN.md 4.15 states the measured ratio to the dense solve's own error).
 * One stated deviation: two waypoints with free end derivatives are solved properly (the reference reads uninitialised
 * memory there, poly_solver.cpp:202-209).
 *
 * Status of a problem: MPLX_SOLVE_EMPTY W < 2 (the reference returns false; n_wp above w_max counts as w_max);
 * MPLX_SOLVE_BAD_TIME a duration that is not finite or <= 0 (a given dt, v <= 0, coincident consecutive waypoints under
 * allocation); MPLX_SOLVE_SINGULAR a pivot of the free system that is not finite or <= 0 (e.g. no position fixed
 * anywhere).  A problem with any bit writes its status only: its other outputs keep the caller's bytes, and samples and
 * traversals skip it as they skip MPLX_TRAJ_EMPTY (mplx_traj.h): nothing sampled, traverse cost 0.0 and counts 0.
 *
 * An mplx_poly holds the K solved trajectories of its last mplx_solve*: segment table, taus, S, T, status, the
 * waypoints, and the workspace of the elimination; all in device memory of its context, sized at creation.  Destroy it
 * before its context.  The _device forms are asynchronous on the context's stream with no host read; the host-pointer
 * twins stage through the context's arena and are synchronous.  Every output pointer is optional.
 *
 * Errors: MPLX_ERR_ARG for NULL poly / in / out, NULL waypoints with n_prob > 0, strides below n_prob, w_max < 2 or
 * above the poly's, n_prob above k_cap, a control other than VEL / ACC / JRK (with or without the yaw bit), a
 * yaw_control other than MPLX_VEL, and what mplx_traj.h lists for times, strides and lanes; MPLX_ERR_STATE for info /
 * sample / traverse before a solve, and for traverse without a map or with v_max <= 0.  n_prob == 0 is a successful
 * no-op. */
#ifndef MPLX_SOLVE_H
#define MPLX_SOLVE_H

#include "mplx.h"
#include "mplx_traj.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_SOLVE_EMPTY = 1, MPLX_SOLVE_BAD_TIME = 2, MPLX_SOLVE_SINGULAR = 8 };  /* (4 is MPLX_TRAJ_BAD of a traversal) */
enum { MPLX_USE_POS = 1, MPLX_USE_VEL = 2, MPLX_USE_ACC = 4 };                    /* waypoint.h:43-50 */

typedef struct mplx_poly mplx_poly;
int mplx_poly_create(mplx_ctx *ctx, int64_t k_cap, int32_t w_max, mplx_poly **out);
void mplx_poly_destroy(mplx_poly *poly);

typedef struct {
  const double *waypoints;  /* field-major state rows: field f of waypoint w of problem k at
                               waypoints[(f * w_max + w) * wp_stride + k], f over the 4D+2 fields pos, vel, acc, jrk, yaw,
                               t: the seg_state layout of mplx_traj_info_out with w_max = horizon + 1                    */
  int64_t n_prob;           /* K                                                                                         */
  int32_t w_max;
  int64_t wp_stride;
  const int32_t *n_wp;      /* [K] W_k, or NULL: w_max each                                                              */
  const double *dts;        /* [w_max - 1][dt_stride], or NULL: allocate_time with v / v_arr                             */
  int64_t dt_stride;
  double v;
  const double *v_arr;      /* [K] or NULL: v for every problem                                                          */
  int32_t control;          /* of the two ends: MPLX_VEL / ACC / JRK, with or without the yaw bit                        */
  int32_t yaw_control;      /* MPLX_VEL                                                                                  */
  const uint8_t *wp_flags;  /* [w_max][flag_stride] MPLX_USE_* bits, or NULL: setPath mode                               */
  int64_t flag_stride;
} mplx_solve_in;

typedef struct {
  uint8_t *status;          /* [K]                                                                                       */
  int32_t *n_segs;          /* [K] S_k                                                                                   */
  double *total_time;       /* [K] T                                                                                     */
  double *coeff;            /* PolyTraj::p(): p[(s N + r) D + i] of problem k at coeff[((s N + r) D + i) * coeff_stride + k];
                               segments past S_k keep the caller's bytes                                                 */
  int64_t coeff_stride;
  double *dts_out;          /* [w_max - 1][dts_out_stride]                                                               */
  int64_t dts_out_stride;
  double *yaw_coeff;        /* the yaw solve's p: [(2 s + r) * yaw_stride + k]                                           */
  int64_t yaw_stride;
  double *taus;             /* [w_max][taus_stride]: taus[0 .. S_k]                                                      */
  int64_t taus_stride;
} mplx_solve_out;

int mplx_solve_device(mplx_poly *poly, const mplx_solve_in *d_in, const mplx_solve_out *d_out);
int mplx_solve(mplx_poly *poly, const mplx_solve_in *h_in, const mplx_solve_out *h_out);

/* On the set the poly holds, with the structs and rules of mplx_traj.h: info (efforts J(VEL), J(ACC), J(JRK), J(SNP) and
 * Jyaw of the solved primitives with their own durations; seg_state = the waypoints, row f of waypoint w at
 * seg_state[(f * w_max + w) * seg_stride + k]), samples (the segment of a time by bisection of the stored taus, then the
 * first-match rules of the two forms), and env_map::traverse_trajectory on the map the context holds NOW: n =
 * ceil(v_max T / res) with the v_max and res of the call. */
int mplx_poly_info_device(mplx_poly *poly, const mplx_traj_info_out *d_out);
int mplx_poly_info(mplx_poly *poly, const mplx_traj_info_out *h_out);
int mplx_poly_sample_device(mplx_poly *poly, const mplx_traj_times *d_times, const mplx_traj_sample_out *d_out);
int mplx_poly_sample(mplx_poly *poly, const mplx_traj_times *h_times, const mplx_traj_sample_out *h_out);
int mplx_poly_traverse_device(mplx_poly *poly, int32_t lanes, const mplx_traj_traverse_out *d_out);
int mplx_poly_traverse(mplx_poly *poly, int32_t lanes, const mplx_traj_traverse_out *h_out);

#ifdef __cplusplus
}
#endif
#endif
