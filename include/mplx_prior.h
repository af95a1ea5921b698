/* mplx_prior.h -- prior-trajectory guidance of an open set (include/mplx_open.h, include/mplx_multi.h): the heuristic
 * of a node follows where a prior trajectory is at the node's own time, and the goal moves to the prior's end.
 * Reference: PlannerBase::setPriorTrajectory -> env_map::set_prior_trajectory (env_map.h:189-226) and env_base::get_heur
 * (env_base.h:46-53); the host restatement set_prior_trajectory of csrc/host_planner.hpp is normative wherever the
 * reference is undefined.  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * 1. The prior table.  An open set of a table with Q queries holds, per query q,
 *   n_steps[q] >= 0        0: no prior -- heuristic and goal of q are exactly those of mplx_open_set_goals
 *   pos[q][k][D], togo[q][k]   for k < n_steps[q]
 *   a replaced goal row and goal hash in its goals[q]
 * in device memory of its own, sized by the host-known bounds step_capacity = ceil(horizon * source.dt / dt) + 2 and
 * ceil(v_max * horizon * source.dt / res) + 3 samples (dt, v_max, res: the searching context's).  mplx_open_clear leaves
 * the priors in force (a replan clears and pushes again); mplx_open_set_goals drops all of them (a new goal: the old prior
 * no longer leads to it); mplx_open_clear_priors drops them and restores the goals of mplx_open_set_goals.  Priors need
 * goals of the open set's own: an open set of one query must have been given mplx_open_set_goals with n == 1.
 *
 * 2. mplx_open_set_priors_device.  d_set: a trajectory set as in include/mplx_traj.h with n_traj == Q; trajectory q is
 * the prior of query q; a first action of -1 (MPLX_TRAJ_EMPTY) means no prior for q.  source: what the prior was planned
 * with -- its control flag, its control table in device memory and its primitive duration; map, potential map and
 * weights, geometry, v_max, w and dt come from the searching context as it is NOW.  Per query, bit for bit
 *   T            the sequential sum of the segment durations (mplx_traj.h)
 *   samples      n = (int)ceil(v_max * T / res); the n + 1 Command samples of sample(n): time stamp k * (T / n), cell index in
 *                wrapping 32-bit arithmetic, |vel|
 *   traverse     env_map.h:229-255, the rule of mplx_traj_traverse_device; total_cost = traverse + w * T
 *   steps        t_0 = 0, t_{k+1} = t_k + dt by sequential addition, while t_k < T: n_steps of them
 *   costs[k]     = w * t_k + P(t_k); P = the sum over the samples with time stamp < t_k, skipping a sample whose cell index
 *                equals the previous sample's, of potential_weight * value + gradient_weight * |vel| (no range test on the
 *                value; a sample outside the map reads 0), one IEEE add per term in sample order; 0 without a potential map
 *   pos[k]       the Waypoint-form evaluation at t_k
 *   togo[k]      = total_cost - costs[(int)(t_k / dt)]: the truncated quotient, not k (with dt = 0.1 the accumulated
 *                t_8 = 0.7999999999999999 gives index 7)
 *   goal         goals[q]'s row becomes the Waypoint at T (the last segment at T - taus[S-1], with t = 0), its hash the lattice
 *                hash of that row under source.control; tolerances, w and v_max stay those of mplx_open_set_goals
 * A prior through an obstacle or out of the map has traverse = +inf and every togo = +inf (the reference's behaviour).
 * MPLX_TRAJ_BAD (sample count not finite or >= 2^31, or past the bounds above) and MPLX_TRAJ_EMPTY give n_steps = 0 and the
 * status; MPLX_TRAJ_BAD_ACTION uses the segments before the bad action.  The call replaces the priors of ALL queries.
 * Asynchronous on the context's stream unless h_info_or_null asks for the per-query status and n_steps (one
 * synchronisation).  Launches: the chain and traverse launches of mplx_traj.h on the source's controls, one lane per
 * sample (cell, map value, |vel|), one lane per trajectory (the two serial chains), one lane per query (goal row, hash).
 * No result depends on how many lanes worked on a trajectory; no multiply-add is contracted.
 *
 * 3. Every push (mplx_open_push_device, mplx_open_push_closed_device, with or without sight) of a row of query q with
 * n_steps[q] > 0 whose hash is not the goal hash: t = row 4D+1 of the state, x = t > 0 ? t / dt : 0; if x < n_steps[q], with
 * k = (int)x: h = w * Linf(pos - pos[q][k]) / v_max + togo[q][k] (w * Linf + togo when v_max <= 0); otherwise (x >= n_steps[q],
 * a NaN x) the goal heuristic, as before.  The key rule and the flags are unchanged.  An open set without priors runs the
 * kernels it ran before this header existed.
 *
 * Errors, each before anything is launched: MPLX_ERR_ARG for NULL o / source / d_set / source->U, nU < 1, udim smaller
 * than the control flag needs, an unknown control flag, dt not > 0, n_traj != Q, horizon < 1, bad strides, a table that
 * would exceed 2^28 entries; MPLX_ERR_STATE without goals of the open set's own, without params, map, or with v_max <= 0
 * or dt <= 0 in the searching context.                                                                              */
#ifndef MPLX_PRIOR_H
#define MPLX_PRIOR_H

#include "mplx_multi.h"
#include "mplx_traj.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t control;   /* the prior's control flag (MPLX_VEL .. MPLX_SNP, with or without the yaw bit) */
  int32_t nU, udim;
  const double *U;   /* device memory, [nU][udim]                                                    */
  double dt;         /* the prior's primitive duration                                               */
} mplx_prior_source;

typedef struct {
  uint8_t *status;   /* host memory [Q]: MPLX_TRAJ_* bits, or NULL */
  int32_t *n_steps;  /* host memory [Q], or NULL                   */
} mplx_prior_info;

/* Device pointers owned by the open set; all NULL / 0 while no prior is in force.  goal_row / goal_hash: the goal every
 * query's pushes use now (the prior's end, or the goal of mplx_open_set_goals).                                       */
typedef struct {
  const int32_t *n_steps;  /* [Q]                          */
  const double *pos;       /* [Q][step_capacity][D]        */
  const double *togo;      /* [Q][step_capacity]           */
  const double *goal_row;  /* [Q][14], 4D+2 meaningful     */
  const uint64_t *goal_hash; /* [Q]                        */
  int64_t step_capacity;
} mplx_prior_view;

int mplx_open_set_priors_device(mplx_open *o, const mplx_prior_source *source, const mplx_traj_set *d_set,
                                const mplx_prior_info *h_info_or_null);
int mplx_open_clear_priors(mplx_open *o);
int mplx_open_prior_view_of(mplx_open *o, mplx_prior_view *v);

/* The prior table of a host planner (mplx_planner_set_prior_trajectory*): *n = its steps; the first min(*n, cap) entries
 * of pos [.][D] and togo, the prior's goal row (4D+2 doubles) and control flag; any output may be NULL.               */
int mplx_planner_prior_table(const mplx_planner *p, double *pos, double *togo, int32_t cap, int32_t *n, double *goal_row,
                             int32_t *control);

#ifdef __cplusplus
}
#endif
#endif
