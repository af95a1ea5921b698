/* mplx_rollout.h -- batched rollouts: cost and validity of K action sequences on the map the context holds NOW.
 * Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * Context state used: map, potential map, search region, mplx_params, control table U -- exactly what
 * mplx_expand_device uses.  Rollout k has a start state s_0 (4D+2 doubles, the Waypoint rows of mplx.h) and actions
 * a_0 .. a_{H-1} (indices into U; -1 ends the sequence early).  For h = 0, 1, ...: the ONE pair (s_h, U[a_h]) is
 * evaluated exactly as get_succ does (reference env_map.h:147-172, :90-132; the same device arithmetic as
 * mplx_expand_device) and its slot status read:
 *   MPLX_SLOT_FINITE   prefix += cost_h (first step: 0.0 + cost_0; one IEEE add per step, in step order -- the order
 *                      in which A* forms g, graph_search.h:107), s_{h+1} = the successor state with t = t_h + dt,
 *                      steps += 1, go on;
 *   SKIP_SAME, BLOCKED, SKIP_DYN   the rollout stops; its status is that slot status;
 *   a_h == -1 or h == H             the rollout is complete; status MPLX_SLOT_FINITE;
 *   a_h < -1 or a_h >= nU           the rollout stops with MPLX_ROLLOUT_BAD_ACTION; U is never read out of range.
 *
 * Outputs per rollout, every pointer optional: status; steps (FINITE steps taken); cost (prefix when complete, else
 * +inf: the convention of mplx_succ.cost); prefix_cost (prefix whatever the status: what an MPC ranks partial
 * progress by); end_state (the state after `steps` steps; the start state when steps == 0); end_hash (its lattice
 * hash, waypoint.h:93-125); end_heur / end_flags of the end state with the meaning these rows have in mplx_succ_lists
 * (default heuristic; bit 0 inside the tolerances, bit 1 the goal's lattice state) -- these two need mplx_set_goal,
 * else MPLX_ERR_STATE.
 *
 * Yaw controls: per-sample heading costs use device trig, as everywhere.  Heading-limit DECISIONS (primitive.h:
 * 504-525) within the context's band of their threshold are not trusted to device trig (the yaw pinning of the
 * expansion calls).  mplx_rollout_device ORs MPLX_ROLLOUT_HEADING_BAND into the status of a rollout that met such a
 * decision; its other outputs are what device trig gave.  mplx_rollout resolves those rollouts itself, stepping them
 * through the pinned dense expansion (what mplx_expand runs), and never returns the bit.
 *
 * Errors: MPLX_ERR_ARG for horizon < 1, n_rollouts < 0, n_starts not in {1, n_rollouts}, strides too small, out ==
 * NULL, NULL starts / actions with n_rollouts > 0; MPLX_ERR_STATE without map / controls / params, or end_heur /
 * end_flags without a goal.  n_rollouts == 0 is a successful no-op.                                               */
#ifndef MPLX_ROLLOUT_H
#define MPLX_ROLLOUT_H

#include "mplx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_ROLLOUT_BAD_ACTION = 4, MPLX_ROLLOUT_HEADING_BAND = 0x80 };

typedef struct {
  uint8_t *status;      /* [n_rollouts] each                                   */
  int32_t *steps;
  double *cost;
  double *prefix_cost;
  double *end_state;    /* field-major [4D+2][end_stride], end_stride >= n_rollouts */
  int64_t end_stride;
  uint64_t *end_hash;   /* [n_rollouts] each                                   */
  double *end_heur;
  uint8_t *end_flags;
} mplx_rollout_out;

/* d_starts: field-major [4D+2][start_stride]; n_starts == n_rollouts, or 1 = every rollout starts at column 0.
 * d_actions: STEP-major, the action of rollout k at step h is d_actions[h * action_stride + k], action_stride >=
 * n_rollouts.  Asynchronous on the context's stream; one kernel launch.  The caller synchronises
 * (mplx_synchronize) before it reads the outputs or overwrites the inputs.                                        */
int mplx_rollout_device(mplx_ctx *ctx, const double *d_starts, int64_t n_starts, int64_t start_stride,
                        const int32_t *d_actions, int64_t n_rollouts, int32_t horizon, int64_t action_stride,
                        const mplx_rollout_out *d_out);
/* The same with host pointers; synchronous.  Never returns MPLX_ROLLOUT_HEADING_BAND.                            */
int mplx_rollout(mplx_ctx *ctx, const double *h_starts, int64_t n_starts, int64_t start_stride,
                 const int32_t *h_actions, int64_t n_rollouts, int32_t horizon, int64_t action_stride,
                 const mplx_rollout_out *h_out);

#ifdef __cplusplus
}
#endif
#endif
