/* mplx_scale.h -- time scaling of the trajectories an mplx_poly holds: Lambda / LambdaSeg, Trajectory::scale,
 * Trajectory::scale_down and the lambda / lambda_dot terms of Trajectory::evaluate on the device.  Exported by
 * libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * Reference: include/mpl_basis/lambda.h (VirtualPoint, LambdaSeg, Lambda), include/mpl_basis/trajectory.h:67-135
 * (evaluate), 140-160 (scale), 165-225 (scale_down), 230-237 (sample), include/mpl_basis/math.h:69-131 (quartic, solve).
 *
 * A Lambda is a positive function lambda(tau) of the virtual time tau in [0, taus[S]] (the time the primitives are
 * written in), piecewise cubic between virtual points (p = lambda, v = lambda', t = tau).  The real time of a virtual
 * time is getT(tau), the integral of lambda from 0 to tau: lambda > 1 slows the motion down.  Ts[s] = getT(taus[s]), the
 * scaled total is Ts[S].  A sample at real time t is the primitives at tau = getTau(t), the inverse of getT, with
 * vel / lambda and the acc / jrk expressions of trajectory.h:119-124.
 *
 * The poly keeps one Lambda per problem: up to MPLX_LAMBDA_MAX_SEGS segments of 8 doubles -- a3, a2, a1, a0 (lambda(tau)
 * = a3 tau^3 + a2 tau^2 + a1 tau + a0 in ABSOLUTE virtual time, LambdaSeg::a), ti, tf, getT(ti) of the segment's own
 * quartic, dT = getT(tf) - getT(ti) --, the segment count, Ts[0 .. S], the scaled total and a status; problem-minor,
 * allocated on first use.  A new solve or load into the poly clears every Lambda; the gather form of mplx_poly_load
 * does not copy the source's.
 *
 * Coefficients.  The reference takes them from Eigen's A.inverse() * b.  Here they are the Hermite cubic through the
 * two points, one stated expression tree (IEEE, -ffp-contract=off):
 *     h = t2 - t1, m = (p2 - p1) / h,
 *     c3 = ((v1 + v2) - 2 m) / (h h),           c2 = ((3 m - 2 v1) - v2) / h,
 *     a3 = c3,                                  a2 = c2 - (3 c3) t1,
 *     a1 = (v1 - (2 c2) t1) + ((3 c3) t1) t1,   a0 = ((p1 - v1 t1) + (c2 t1) t1) - ((c3 t1) t1) t1.
 * dT, getT and Ts are lambda.h:57-60, 127-138 operation for operation (power() by repeated multiplication).
 *
 * Two modes, as include/mplx_limits.h has for the same reason.  MPLX_SCALE_REFERENCE says what the reference says;
 * MPLX_SCALE_ROBUST is right.  What the reference does, found by compiling its headers and sweeping them on a CPU:
 *   1. scale_down does not compile if instantiated: it calls extrema_vel and Primitive1D::evaluate, which do not exist.
 *      mplx_poly_scale_down is therefore a restatement, defined below, in both modes.
 *   2. Lambda::getTau loses the end points.  It inverts the time map with the closed-form quartic() of math.h and takes
 *      the first root inside [ti, tf].  At interior times it finds a root, a poor one: |getT(tau) - t| reaches 1.3e-6 of
 *      the scaled duration.  At t = 0, t = total and at N * (total / N), the last sample of sample(N), it finds none in
 *      about a third of random scale(ri, rf) calls and returns -1; evaluate then clamps -1 to 0, so the last sample of
 *      sample(N) is the START state.  REFERENCE does exactly this (found = 0).
 *   3. LambdaSeg zeroes every coefficient with |a| < 1e-5.  On long trajectories (2 |dp| / h^3 < 1e-5) that removes the
 *      cubic term: lambda(tf) is then wrong by more than 0.1 %, and with dp < 0 lambda can turn negative, so time runs
 *      backwards.  REFERENCE applies the clamp; ROBUST does not.
 *   4. evaluate clamps tau to [0, total_t_], and total_t_ is the SCALED total after scale(): a trajectory that was sped
 *      up (total < taus[S]) is cut short at tau = total.  REFERENCE clamps so; ROBUST clamps to [0, taus[S]].  (A tau the
 *      reference's clamp lets past taus[S] is evaluated on the last segment; the reference returns false there.)
 *   5. scale_down places virtual points only at velocity extrema, so the ramps up to the plateau are never checked
 *      against the limit; it looks at velocity only; its loop over axes runs i < 3 also in 2-D.  The restatement below
 *      checks acceleration too and loops i < D.  ITS RAMPS ARE NOT CHECKED AGAINST THE LIMITS EITHER, as the
 *      reference's are not: only ri <= 0 and rf <= 0 (no ramps: a uniform scaling) is within mv and ma by construction.
 *
 * mplx_poly_set_lambda: Lambda(vs) from caller-given virtual points: rows p, v, t of point j of problem k at
 * pts[(j * 3 + {0, 1, 2}) * stride + k], j < n_pts[k] (NULL: 9 each), in order.  The points should span [0, taus[S]].
 *   REFERENCE: the 1e-5 clamp; MPLX_LAMBDA_BAD_POINTS for fewer than 2 or more than 9 points or a value that is not
 *     finite; nothing else is validated.
 *   ROBUST: no clamp.  MPLX_LAMBDA_BAD_POINTS also for times that do not grow strictly and for p <= 0;
 *     MPLX_LAMBDA_NOT_POSITIVE when the cubic of a segment is <= 0 at an end or at a root of its derivative inside the
 *     segment (quad of math.h on 3 a3, 2 a2, a1; the linear root when a3 == 0).
 *   A problem with a status has no Lambda (it is sampled unscaled), and writes its status only: its other outputs keep
 *   the caller's bytes.  Problems with a solve or load status are skipped altogether.
 *
 * mplx_poly_scale: Trajectory::scale(ri, rf): the points (1 / ri, 0, 0) and (1 / rf, 0, taus[S]); ri / rf per problem
 * (ri_arr / rf_arr) or the scalars.  ri or rf that is <= 0 or not finite: MPLX_LAMBDA_BAD_POINTS in both modes.
 *
 * mplx_poly_scale_down(mv, ma, ri, rf).  Velocity is checked when mv > 0, acceleration when ma > 0; jerk is left out
 * (the reference's Command scales jerk by lambda^2, so no consistent rule exists).  For every segment s and axis i < D
 * whose axis_max<order, ALL_ROOTS> (mplx_limits.h) exceeds the limit, the candidates are the extrema that rule set
 * looks at inside (0, dt), 0 for s != 0, and dt.  A candidate at tv with value x has l = |x| / mv (velocity) or
 * sqrt(|x| / ma) (acceleration); one with l > 1 is recorded as (taus[s] + tv, l).  max_l, t_lo, t_hi: the largest l, the
 * smallest and the largest recorded time.  Per-segment results come from one lane per (problem, segment), then one
 * ordered pass per problem: a pure function of the inputs.  No record: the problem is left unscaled (it has no Lambda
 * afterwards), scaled[k] = 0 -- the reference returns false.  Otherwise the points are (ri, 0, 0), (max_l, 0, t_lo),
 * (max_l, 0, t_hi) if t_hi > t_lo, (rf, 0, T) if T > t_hi: a violation at T itself wins over rf.  ri and rf are LAMBDA
 * VALUES here, not ratios, as in the reference's scale_down; ri <= 0 / rf <= 0 means "max_l": no ramp at that end.  The
 * Lambda is then built as by mplx_poly_set_lambda in the mode given.  When NO problem was scaled the host form leaves
 * the poly a plain one (as after mplx_poly_clear_lambda); the _device form reads nothing back and cannot know: the poly
 * then counts as scaled although every problem is sampled unscaled -- traverse is refused and samples run the Lambda
 * instantiation -- until mplx_poly_clear_lambda, which a caller who reads `scaled` back should call.
 *
 * mplx_poly_tau: the inverse map for arbitrary real times (mplx_traj_times; its form is not read), one lane per
 * (problem, time): tau = getTau(t) as it comes (REFERENCE: -1 where no root was found), lambda and lambda_dot =
 * Lambda::evaluate at that tau clamped as a sample clamps it, found.  Element i of problem k at [k * stride + i].
 *   REFERENCE: Lambda::getTau expression for expression: the first segment with t >= T && t <= T + dT, solve(a3 / 4,
 *     a2 / 3, a1 / 2, a0, T - t - getT(ti)), the first returned root in [ti, tf], else on to the next segment.
 *   ROBUST: t <= 0 -> 0 and t >= total -> taus[S] exactly; else the segment by the cumulative dT, a start from the
 *     closed-form root nearest [ti, tf] (the linear guess when there is none), clamped to [ti, tf], then
 *     MPLX_LAMBDA_NEWTON steps tau -= ((getT(tau) - getT(ti)) + T0 - t) / lambda(tau), each clamped to [ti, tf].  A fixed
 *     count, no data-dependent loop.  found is always 1.
 *   Lambda::evaluate(tau): the first segment with tau >= ti && tau < tf; none: lambda = lambda_dot = 0 in REFERENCE (the
 *     reference's VirtualPoint there is not even initialised), the last segment in ROBUST.
 *   A problem without a Lambda: tau = t, lambda = 1, lambda_dot = 0, found = 1.  A time that is not finite: NaN, found 0.
 *
 * On a poly that holds a Lambda: mplx_poly_sample uses tau = getTau(time) under the Lambda's mode, clamped (quirk 4),
 * then Lambda::evaluate(tau), then the Command expressions of trajectory.h:119-124 with that lambda and lambda_dot;
 * Waypoints are the primitives at tau as they are (trajectory.h:67-90 does not use lambda).  Uniform sampling is i *
 * (total_scaled / N); under a ROBUST Lambda sample N is total_scaled itself (N * (total / N) can fall an ulp short of
 * it), so the last sample is the END state; mplx_poly_tau's uniform times are the same.  mplx_poly_info reports the
 * scaled total; efforts stay those of the primitives (the reference's J ignores lambda).  mplx_poly_limits stays the
 * primitives' limits.  mplx_poly_traverse returns MPLX_ERR_STATE: time scaling does not move the path, traverse it
 * before scaling or after mplx_poly_clear_lambda.
 *
 * The _device forms are asynchronous on the context's stream with no host read; the host-pointer twins stage through
 * the context's arena and are synchronous.  A poly counts as holding a Lambda once the launches of a build are queued;
 * a build that fails before that leaves it a plain one.  Every output pointer is optional.
 *
 * Errors: MPLX_ERR_ARG for NULL poly / in / out, NULL pts with problems to read, strides below n_prob (tau: below the
 * sample count), a mode other than the two, bad times (mplx_traj.h); MPLX_ERR_STATE before any solve or load, for
 * mplx_poly_tau on a poly without a Lambda, and for traverse on a poly with one.  A solve or load with n_prob == 0 is a
 * no-op, as ever: the poly keeps the set and the Lambda it held. */
#ifndef MPLX_SCALE_H
#define MPLX_SCALE_H

#include "mplx_limits.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_SCALE_REFERENCE = 0, MPLX_SCALE_ROBUST = 1 };
enum { MPLX_LAMBDA_BAD_POINTS = 32, MPLX_LAMBDA_NOT_POSITIVE = 64 };
enum { MPLX_LAMBDA_MAX_SEGS = 8, MPLX_LAMBDA_NEWTON = 3 };

typedef struct {
  uint8_t *status;     /* [K] 0, MPLX_LAMBDA_BAD_POINTS or MPLX_LAMBDA_NOT_POSITIVE                                      */
  int32_t *n_lseg;     /* [K] segments of the Lambda                                                                     */
  double *total;       /* [K] the scaled total, Ts[S]                                                                    */
  double *Ts;          /* [w_max][ts_stride]: Ts[0 .. S_k]                                                               */
  int64_t ts_stride;
  double *segs;        /* field f (a3 a2 a1 a0 ti tf getT(ti) dT) of segment s at segs[(s * 8 + f) * seg_stride + k]     */
  int64_t seg_stride;
} mplx_lambda_out;

typedef struct {
  const double *pts;   /* [9][3][stride]                                                                                 */
  int64_t stride;
  const int32_t *n_pts; /* [K] or NULL: 9 each                                                                           */
  int32_t mode;
} mplx_lambda_in;

int mplx_poly_set_lambda_device(mplx_poly *poly, const mplx_lambda_in *d_in, const mplx_lambda_out *d_out);
int mplx_poly_set_lambda(mplx_poly *poly, const mplx_lambda_in *h_in, const mplx_lambda_out *h_out);

typedef struct {
  double ri, rf;       /* ratios at the start and the end                                                                */
  const double *ri_arr, *rf_arr;  /* [K] each, or NULL: the scalar                                                       */
  int32_t mode;
} mplx_scale_in;

int mplx_poly_scale_device(mplx_poly *poly, const mplx_scale_in *d_in, const mplx_lambda_out *d_out);
int mplx_poly_scale(mplx_poly *poly, const mplx_scale_in *h_in, const mplx_lambda_out *h_out);

typedef struct {
  double mv, ma;       /* <= 0: not checked                                                                              */
  double ri, rf;       /* lambda at the start and the end; <= 0: max_l                                                   */
  int32_t mode;
} mplx_scale_down_in;

typedef struct {
  uint8_t *scaled;     /* [K] 1: a Lambda was built (see lambda.status), 0: within the limits, left unscaled             */
  double *max_l, *t_lo, *t_hi;  /* [K] each; written where scaled is 1                                                   */
  mplx_lambda_out lambda;
} mplx_scale_down_out;

int mplx_poly_scale_down_device(mplx_poly *poly, const mplx_scale_down_in *in, const mplx_scale_down_out *d_out);
int mplx_poly_scale_down(mplx_poly *poly, const mplx_scale_down_in *in, const mplx_scale_down_out *h_out);

typedef struct {
  double *tau, *lambda, *lambda_dot;
  uint8_t *found;
  int64_t stride;      /* >= the sample count (N + 1 or Q)                                                               */
} mplx_tau_out;

int mplx_poly_tau_device(mplx_poly *poly, const mplx_traj_times *d_times, const mplx_tau_out *d_out);
int mplx_poly_tau(mplx_poly *poly, const mplx_traj_times *h_times, const mplx_tau_out *h_out);

/* every problem of the poly is unscaled again (a switch on the host: nothing is launched) */
int mplx_poly_clear_lambda(mplx_poly *poly);

#ifdef __cplusplus
}
#endif
#endif
