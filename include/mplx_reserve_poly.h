/* mplx_reserve_poly.h -- polynomial trajectories against a reservation table: the check that mplx_reserve_check_device
 * (include/mplx_reserve.h) makes for list entries, made for the problems of a solved or loaded set on the table's
 * common clock, and the shortcut that admits only hops which stay clear of the reservations.  Exported by libmplx.so
 * next to include/mplx.h, whose ABI version it does not change.  The reference has nothing of the kind; what is
 * normative is stated here and restated sequentially in tests/reserve_poly_model.py.
 *
 * All arithmetic is IEEE double under -ffp-contract=off, in the order written.
 *
 * Check.  mplx_reserve_check_poly_device looks at the K problems of `poly` (its last solve or load) against the table
 *   of `res` (B reserved trajectories, n_steps instants at (double)i * step; include/mplx_reserve.h).  For problem k:
 *     t_start[k]  the clock time of the trajectory's local time 0;
 *     r_k         radius[k], or radius_all without `radius`;
 *     ign_k       ignore_group[k], or -1 without `ignore_group`;
 *     total_k     the problem's total time: the scaled total where the problem holds a Lambda (include/mplx_scale.h),
 *                 else the T of its table;
 *     tl_i        = (double)i * step - t_start[k].
 *   Excluded.  A problem with any status bit of the set or with S == 0 segments, one whose t_start is not finite and
 *              one whose radius is negative or not finite.  The latter two get MPLX_CONFLICT_BAD_INPUT in status[k].  An
 *              excluded problem has hit = -1; nothing of it is evaluated.
 *   Horizon.   If (double)(n_steps - 1) * step - t_start[k] < total_k the problem leaves the table's horizon: hit = -2 and
 *              no pair test is made.  Nothing passes unchecked.
 *   Instants.  Otherwise: every i in [0, n_steps) with tl_i >= 0 && tl_i <= total_k.  Closed at both ends: the active rule
 *              of MPLX_CONFLICT_GONE.  A problem that falls between two instants has none.  (The kernel finds the first
 *              one from a guess, t_start / step, and a scan of at most 4 instants, then walks upwards while
 *              tl_i <= total_k; tl_i is monotone in i and the set is the one stated, however it is found.)
 *   Position.  At instant i: bit for bit what the position launch of include/mplx_conflict.h computes for this set
 *              with t0 = t_start -- local time tl_i, scale::sample_tau under the Lambda's mode where the problem holds
 *              one, traj::find_segment and traj::eval_segment on the solved segments -- i.e. the position
 *              mplx_poly_sample gives at tl_i in Command form.
 *   Pair test. The check's: against every b of the table that is included, active at i and has group[b] != ign_k:
 *              dx = pos_k - pos_b per axis, d2 = (dx * dx) + dy * dy (+ dz * dz), rr = r_k + radius[b]; a conflict iff
 *              d2 < rr * rr.  Strict: touching is none.  A d2 that is NaN is no conflict.
 *   Result.    hit[k] = the minimum of ((int64)i << 32 | b) over the problem's conflicts, -1 without one, -2 for the
 *              horizon.  status[k] = the set's status bits of problem k | MPLX_CONFLICT_BAD_INPUT.  *n_hit is increased by
 *              the number of problems with hit != -1.  Every pointer of the out struct is optional.
 *   Every output is a minimum or a sum of integers: a pure function of the inputs whatever the tiling.  Nothing of the
 *   poly or of the table is written.
 *
 * The _device form runs asynchronously on the context's stream with no host read; the host-pointer twin copies its
 * [K] rows through a row buffer that the reservation table owns (not the context's staging arena) and is synchronous.
 *
 * Errors: MPLX_ERR_ARG for NULL res / poly / in / out / t_start and a poly of another context; MPLX_ERR_STATE for a check
 * before a fill and for a poly without a solve or load.  mplx_reserve_set_queries is not needed.  K == 0 is a no-op.
 *
 * Timed shortcut.  mplx_shortcut_timed_device is mplx_shortcut_device (include/mplx_limits.h) with one more admission
 *   rule.  The queries of `res` (mplx_reserve_set_queries: t0, radius, ignored group) are the shortcut's queries; their
 *   number must be n_query, else MPLX_ERR_ARG.  After the pair solve the pair set is checked as above: pair
 *   p = (k, i, j) has t_start = t0[k] + t_i (one IEEE add, t_i the t row of chain state i), radius[k] and ignore[k].
 *     A non-adjacent edge is admitted iff the conditions of mplx_shortcut_device hold AND its hit == -1: the horizon
 *       blocks it too.
 *     An adjacent edge stays always admitted: the search validated it with its own primitive, and the re-solved
 *       polynomial equals that primitive only up to rounding.
 *     chain_hit[k] (optional, [n_query] int64) = the smallest hit >= 0 of the query's adjacent edges i -> i + 1,
 *       i + 1 < W_k, or -2 if none is >= 0 and one leaves the horizon, or -1: a chain that no longer holds against the
 *       table as it is now is reported, not hidden.
 *   Everything else -- inputs, outputs, costs, the programme, the gather into `result` -- is mplx_shortcut_device's.
 *   Chains with wait edges (repeated states with t_{i+1} > t_i) are legal in both shortcuts: a rest pair is a
 *   two-waypoint solve with positive duration whose polynomial is the constant.
 *   Errors: those of mplx_shortcut_device; NULL res, a table of another context or a number of queries other than
 *   n_query: MPLX_ERR_ARG; before a fill or before mplx_reserve_set_queries: MPLX_ERR_STATE.  Asynchronous, no host read.
 *   The host-pointer twin copies the rows mplx_shortcut stages, through the reservation table's own row buffer. */
#ifndef MPLX_RESERVE_POLY_H
#define MPLX_RESERVE_POLY_H

#include "mplx_limits.h"
#include "mplx_reserve.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  const double *t_start;       /* [K] clock time of the trajectory's local time 0; finite, may be negative */
  const double *radius;        /* [K] or NULL: radius_all each; finite, >= 0                                */
  double radius_all;
  const int32_t *ignore_group; /* [K] or NULL: -1 each                                                      */
} mplx_reserve_poly_in;

typedef struct {
  int64_t *hit;                /* [K] min of ((int64)i << 32 | b) over the conflicts, -1 none, -2 horizon   */
  uint8_t *status;             /* [K] the set's status bits | MPLX_CONFLICT_BAD_INPUT                       */
  int64_t *n_hit;              /* one counter, increased by the problems with hit != -1                     */
} mplx_reserve_poly_out;       /* every pointer optional */

int mplx_reserve_check_poly_device(mplx_reserve *res, mplx_poly *poly, const mplx_reserve_poly_in *d_in,
                                   const mplx_reserve_poly_out *d_out);
/* Host pointers; *n_hit is read, increased and written back.                                                         */
int mplx_reserve_check_poly(mplx_reserve *res, mplx_poly *poly, const mplx_reserve_poly_in *h_in,
                            const mplx_reserve_poly_out *h_out);

int mplx_shortcut_timed_device(mplx_poly *pairs, mplx_poly *result, const mplx_shortcut_in *d_in, const mplx_shortcut_out *d_out,
                               mplx_reserve *res, int64_t *d_chain_hit_or_null);
int mplx_shortcut_timed(mplx_poly *pairs, mplx_poly *result, const mplx_shortcut_in *h_in, const mplx_shortcut_out *h_out,
                        mplx_reserve *res, int64_t *h_chain_hit_or_null);

#ifdef __cplusplus
}
#endif
#endif
