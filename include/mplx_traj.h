/* mplx_traj.h -- Trajectory<Dim> on the device: sample, evaluate, J / Jyaw, and env_map::traverse_trajectory on the
 * map the context holds NOW.  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * A trajectory set is described exactly as mplx_rollout describes its input (the same device buffers serve both).
 * Trajectory k has S_k segments: its actions before the first -1, or `horizon` of them.  Control flag, dt, v_max, the
 * weights and the control table U come from the context.  Reference: include/mpl_basis/trajectory.h,
 * include/mpl_basis/primitive.h, include/mpl_planner/env/env_map.h:229-255; bit for bit its arithmetic.
 *
 *   s_0            = the start state; s_{s+1} = Primitive(s_s, U[a_s], dt).evaluate(dt) with t + dt (env_map.h:156-161):
 *                    the state the search stores and recoverTraj rebuilds.  NO validity check: kinematics only.
 *   taus[0] = 0,   taus[s+1] = dt + taus[s] by sequential addition (trajectory.h:52-56); T = taus[S].
 *   a_s < -1 or a_s >= nU   the build stops: MPLX_TRAJ_BAD_ACTION, the trajectory is the segments before the bad action;
 *                    U is never read out of range.
 *   S_k == 0        MPLX_TRAJ_EMPTY: T = 0, efforts 0, traverse cost 0.0, nothing is sampled (the reference divides 0 by
 *                    0 there).
 *
 * Every call builds the segment table of its set first (one launch into scratch memory of the context) and then runs
 * on it; the _device forms are asynchronous on the context's stream with no host read between their launches, the
 * host-pointer twins stage through the context's arena and are synchronous.  Every output pointer is optional.
 *
 * Errors: MPLX_ERR_ARG for a NULL context, set or out, NULL starts / actions with n_traj > 0, strides smaller than
 * the counts, horizon < 1, n_starts not in {1, n_traj}, N < 1 / Q < 1, an unknown form or lanes; MPLX_ERR_STATE
 * without params / controls, and for traverse without a map or with v_max <= 0.  n_traj == 0 is a successful no-op. */
#ifndef MPLX_TRAJ_H
#define MPLX_TRAJ_H

#include "mplx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status bits of a trajectory */
enum { MPLX_TRAJ_EMPTY = 1, MPLX_TRAJ_BAD_ACTION = 2, MPLX_TRAJ_BAD = 4 };
/* sample forms */
enum { MPLX_TRAJ_COMMAND = 0, MPLX_TRAJ_WAYPOINT = 1 };

typedef struct {
  const double *starts;   /* field-major [4D+2][start_stride]; n_starts == n_traj, or 1 = every trajectory starts at column 0 */
  int64_t n_starts, start_stride;
  const int32_t *actions; /* STEP-major: trajectory k at step h = actions[h * action_stride + k]; -1 ends              */
  int64_t n_traj;
  int32_t horizon;
  int64_t action_stride;
} mplx_traj_set;

/* ---- 1. per trajectory: status, segments, total time, efforts, chain states */
typedef struct {
  uint8_t *status;      /* [n_traj] EMPTY | BAD_ACTION                                                                */
  int32_t *n_segs;      /* [n_traj] S_k                                                                               */
  double *total_time;   /* [n_traj] T = taus[S_k]                                                                     */
  double *effort;       /* [5][effort_stride]: J(VEL), J(ACC), J(JRK), J(SNP), Jyaw.  Trajectory::J is j = 0; j += seg.J(c)
                           in segment order, Primitive::J j = 0; j += pr.J(t, c) in axis order, Primitive1D::J the
                           expression trees of primitive.h:92-122; Jyaw the VEL formula on the yaw primitive               */
  int64_t effort_stride;
  double *seg_state;    /* the S_k + 1 chain states: row f of state s of trajectory k at
                           seg_state[(f * (horizon + 1) + s) * seg_stride + k]; states past S_k keep the caller's bytes  */
  int64_t seg_stride;
} mplx_traj_info_out;
int mplx_traj_info_device(mplx_ctx *ctx, const mplx_traj_set *d_set, const mplx_traj_info_out *d_out);
int mplx_traj_info(mplx_ctx *ctx, const mplx_traj_set *h_set, const mplx_traj_info_out *h_out);

/* ---- 2. samples.  Times: n_uniform = N >= 1: sample i = 0 .. N at i * (T / N) (trajectory.h:230-237; times is
 * ignored); n_uniform == 0: the n_times = Q >= 1 values of `times`, shared by all trajectories (time_stride == 0: times[i])
 * or one column per trajectory (time_stride >= Q: times[k * time_stride + i]).  tau = the time clamped to [0, T].
 *   MPLX_TRAJ_COMMAND (trajectory.h:99-135): the segment is the FIRST id with tau >= taus[id] && tau <= taus[id+1]; rows
 *     pos, vel, acc, jrk (D each), yaw, yaw_dot, t (the unclamped time): 4D+3 rows.  yaw and yaw_dot are normalize_angle of
 *     the yaw primitive's p and v; vel, acc, jrk take the reference's lambda = 1, lambda_dot = 0 expressions.
 *   MPLX_TRAJ_WAYPOINT (trajectory.h:67-90): the first id with tau >= taus[id] && tau < taus[id+1], else the last; writes
 *     the first 4D+1 rows and leaves the other two as the caller had them.
 * Row r, trajectory k, sample i is out[r * row_stride + k * sample_stride + i].  A non-finite time writes NaN into that
 * sample's rows.  Entries past n_traj or the sample count, and every sample of an EMPTY trajectory, keep the caller's
 * bytes.                                                                                                            */
typedef struct {
  int32_t form;
  int32_t n_uniform;
  const double *times;
  int64_t n_times, time_stride;
} mplx_traj_times;
typedef struct {
  double *out;
  int64_t row_stride;     /* >= n_traj * sample_stride                 */
  int64_t sample_stride;  /* >= the sample count (N + 1 or Q)          */
  uint8_t *status;        /* [n_traj] as in mplx_traj_info_out, or NULL */
} mplx_traj_sample_out;
int mplx_traj_sample_device(mplx_ctx *ctx, const mplx_traj_set *d_set, const mplx_traj_times *d_times,
                            const mplx_traj_sample_out *d_out);
int mplx_traj_sample(mplx_ctx *ctx, const mplx_traj_set *h_set, const mplx_traj_times *h_times,
                     const mplx_traj_sample_out *h_out);

/* ---- 3. env_map::traverse_trajectory (env_map.h:229-255).  n = (int)ceil(v_max * T / res), then the n + 1 Command
 * samples of sample(n).  Per sample pn = floatToInt(pos) and idx = getIndex(pn) in 32-bit wrapping int arithmetic, ALSO
 * for cells outside (a coordinate the reference could not convert saturates).  idx == the previous sample's idx (-1
 * before the first) skips the sample before anything else is asked: an outside cell whose index aliases the previous
 * in-map cell is skipped.  Then: outside -> +inf.  With a potential map: a value in (0, 100) adds potential_weight *
 * value + gradient_weight * |vel| (sqrt of the squares summed in axis order), >= 100 -> +inf, -1 and 0 add nothing.
 * Without one: a cell == 100 of the int8 map -> +inf.  The search region is not consulted.  The sum is formed in sample
 * order, one IEEE add per counted sample that adds.  A trajectory whose ceil(v_max * T / res) is not finite or >= 2^31 is
 * MPLX_TRAJ_BAD: cost NaN, counts 0, nothing traced.
 * lanes: 0 (automatic) or 4 / 16 / 64 lanes of a wavefront per trajectory; the results never depend on it.          */
typedef struct {
  uint8_t *status;       /* [n_traj] EMPTY | BAD_ACTION | BAD                                       */
  double *cost;          /* [n_traj]                                                                */
  int32_t *n_samples;    /* [n_traj] n + 1 (0: EMPTY or BAD)                                        */
  int32_t *n_cells;      /* [n_traj] samples counted (not skipped), the one that made the cost +inf included */
  int32_t *stop_sample;  /* [n_traj] index of the sample that made the cost +inf, else -1           */
} mplx_traj_traverse_out;
int mplx_traj_traverse_device(mplx_ctx *ctx, const mplx_traj_set *d_set, int32_t lanes, const mplx_traj_traverse_out *d_out);
int mplx_traj_traverse(mplx_ctx *ctx, const mplx_traj_set *h_set, int32_t lanes, const mplx_traj_traverse_out *h_out);

#ifdef __cplusplus
}
#endif
#endif
