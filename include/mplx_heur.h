/* mplx_heur.h -- dynamics-aware heuristics: what PlannerBase::setHeurIgnoreDynamics(false) switches on in the reference
 * (env_base<Dim>::cal_heur, include/mpl_planner/common/env_base.h:56-211), for batches of states, for the pushes of an
 * open set (include/mplx_open.h) and for the host planner.  Exported by libmplx.so next to include/mplx.h, whose ABI
 * version it does not change.
 *
 * 1. The quantity.  cal_heur is the cost of the unconstrained optimal-control connection from the state to the goal,
 * minimised over the arrival time t >= t_bar = Linf(pos - goal.pos) / v_max.  With dp = goal.pos - pos, v0 / a0 the
 * state's and v1 / a1 the goal's velocity / acceleration (control = the state's flag, goal control = the goal's):
 *   VEL, VEL          C(t) = |dp|^2 / t + w t                                    (this library's; see REFERENCE below)
 *   ACC, ACC / VEL    C(t) = -c1/3/t/t/t - c2/2/t/t - c3/t + w t                 c1 c2 c3 of env_base.h:163-165 / :188-190
 *   JRK, JRK/ACC/VEL  C(t) = a t - c/t - d/2/t/t - e/3/t/t/t - f/4/t/t/t/t - g/5/t/t/t/t/t
 *                                                                                env_base.h:75-81 / :106-111 / :136-140
 * The stationary points of C are the positive roots of  w t^4 + c3 t^2 + c2 t + c1  (ACC)  and of
 * a t^6 + c t^4 + d t^3 + e t^2 + f t + g  (JRK).
 *
 * 2. Modes.
 *   MPLX_HEUR_DEFAULT    w Linf / v_max (w Linf for v_max <= 0): env_base.h:58-64, what every call computed before this
 *                        header existed and still computes while the mode is off.
 *   MPLX_HEUR_REFERENCE  what the reference returns, expression for expression, for the branches that need no Eigen
 *                        solver: ACC-ACC, ACC-VEL, VEL-VEL ((w + 1) L2) and the final else (w L2 / v_max).  Control flags
 *                        are compared exactly, so ACCxYAW falls into the else.  The candidates are those of the reference's
 *                        closed-form quartic in its order, then t_bar; the start value is DBL_MAX; v_max divides as
 *                        written.  It is NOT admissible, even for an exact goal state (the quartic takes the resolvent's
 *                        first root and gives up when r < 0: it misses minima; DESIGN.md 4.23 has the numbers), and it goes
 *                        through cbrt / acos / cos, whose last bits differ between the C library and the device's and flip
 *                        `t < t_bar`.  HOST ONLY: it exists so that the host planner stays search-for-search the
 *                        reference's with the setter on.  A JRK or SNP state space is refused (MPLX_ERR_STATE), not
 *                        approximated: the reference's JRK branches keep a root of Eigen's PolynomialSolver only when its
 *                        imaginary part is exactly 0.
 *   MPLX_HEUR_ROBUST     the true minimum.  Base control = the flag without its yaw bit, of the state and of the goal;
 *                        goal_control == 0 means the state's.  t_bar = v_max > 0 ? Linf / v_max : 0.
 *                          h0 = the default;  m = min of C over {t_bar if t_bar > 0} and {stationary points > t_bar}
 *                          h  = m > h0 ? m : h0          (no candidate, or a pair not listed in 1.: h0)
 *                        so ROBUST is never below the default, bit for bit, and where dynamics add nothing the key is
 *                        the default's.  SNP states and a goal with more derivatives than the state take h0 (not the
 *                        reference's w L2 / v_max, which is no lower bound).  Any non-finite pos / vel / acc row of the
 *                        state or the goal, w or v_max gives NaN.  Only + - * / sqrt fabs and comparisons: the same bits
 *                        on the device, on the host and in tests/heur_model.py, which is its specification.  The roots: all
 *                        real roots in (t_bar, T_hi], T_hi = 1 + max |p_k / p_N| (Cauchy), by the chain of derivatives --
 *                        between two neighbouring roots of p' the polynomial is monotone, a sign change is one root,
 *                        MPLX_HEUR_BISECT halvings find it.  There can be three stationary points; all are looked at.
 * In every mode the goal's own lattice state (its hash under the state's flag equals the goal's under its own,
 * env_base.h:47) has h = 0, unless h is NaN.
 *
 * 3. Admissibility of ROBUST.  A feasible trajectory to the goal STATE lasts at least t_bar (no axis exceeds v_max), and
 * for its duration t its effort is at least the unconstrained optimum, so its cost is at least C(t) >= min over
 * t >= t_bar.  Where it stops: the goal tolerance box and a free goal velocity (an ACC goal whose tol_vel < 0) make any
 * fixed-goal bound approximate, exactly as they do for the default heuristic beyond tol_pos.
 *
 * 4. Calls.  mplx_heur_eval: h_states are K columns of 4D+2 rows (pos vel acc jrk yaw t), row stride `stride` >= K
 * doubles; h_out [K].  The goal spec's tolerances are not read.  It copies the rows through a device block of its own (not the
 * staging arena the other host-pointer calls share) and synchronises.
 * mplx_heur_eval_device: the same on resident rows [4D+2][stride] -- the layout of the table and the frontiers -- one
 * lane per state, asynchronous on the context's stream; it returns h only (goal flags stay the expansion's and the
 * push's).  MPLX_HEUR_REFERENCE is MPLX_ERR_ARG in both: the device takes DEFAULT and ROBUST.
 * mplx_open_set_heur(o, mode): DEFAULT or ROBUST.  While ROBUST is in force every push (mplx_open_push_device,
 * mplx_open_push_closed_device, with or without sight, one query or several) takes h of a row that is not its goal's own
 * lattice state from ROBUST, with the goal, w, v_max, control and goal_control of the row's query's goal
 * (mplx_set_goal / mplx_open_set_goals).  A row whose h is NaN is ignored like any row whose key is not >= 0.  With a
 * goal field (include/mplx_field.h) both bounds hold and the key takes the larger: h = max(h_robust, the field's h), +inf
 * on a cell no chain leaves.  With priors (include/mplx_prior.h) the mode is refused, whichever is set second: the prior
 * table holds positions only.  mplx_open_clear keeps the mode; destroying the open set drops it.  An open set whose
 * mode is DEFAULT runs the kernels it ran before this header existed.
 *
 * mplx_planner_set_heur_dynamics(p, mode): the host planner, A* and LPA* alike (PlannerBase::setHeurIgnoreDynamics):
 * DEFAULT, REFERENCE or ROBUST for every node the next mplx_planner_plan evaluates, with the planner's control, the
 * goal's control, w and v_max.  While a mode other than DEFAULT is on the planner evaluates new nodes itself even if
 * mplx_planner_use_device_heuristic is set: the lists' heur row stays the default heuristic.  With REFERENCE the plan is
 * search for search the reference's MapPlanner with setHeurIgnoreDynamics(false) (tests/golden/heur_golden.npz).  A prior
 * trajectory together with a mode other than DEFAULT is refused, whichever is set second (the planner's prior table
 * holds positions only; the reference's cal_heur(state, prior[id]) + togo, env_base.h:50, is not built).
 *
 * Errors: MPLX_ERR_ARG for NULL required pointers, K < 0, stride < K, an unknown mode, REFERENCE where the device would
 * compute it, an unknown control flag, and w <= 0 or NaN with a mode other than DEFAULT where the mode is set and w is
 * known (mplx_heur_eval*; mplx_open_set_heur with a goal); MPLX_ERR_STATE for the same found later (a push whose goal
 * came after the mode; mplx_planner_plan, which is where the planner's w arrives), for ROBUST or REFERENCE together with
 * priors, and for mplx_planner_plan with REFERENCE on a JRK or SNP state space.  K == 0 is a successful no-op.  No call
 * writes past h_out[K - 1] or loops without a bound.                                                                  */
#ifndef MPLX_HEUR_H
#define MPLX_HEUR_H

#include "mplx_open.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_HEUR_DEFAULT = 0, MPLX_HEUR_REFERENCE = 1, MPLX_HEUR_ROBUST = 2 };
#define MPLX_HEUR_BISECT 56

int mplx_heur_eval(mplx_ctx *ctx, const mplx_goal_spec *goal, int32_t mode, const double *h_states, int64_t K, int64_t stride,
                   double *h_out);
int mplx_heur_eval_device(mplx_ctx *ctx, const mplx_goal_spec *goal, int32_t mode, const double *d_states, int64_t K,
                          int64_t stride, double *d_out);
int mplx_open_set_heur(mplx_open *o, int32_t mode);
int mplx_planner_set_heur_dynamics(mplx_planner *p, int32_t mode);

#ifdef __cplusplus
}
#endif
#endif
