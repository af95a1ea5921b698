/* mplx_limits.h -- caller-given trajectories in an mplx_poly, and the dynamic limits of the set a poly holds:
 * Primitive(cs, t, control) / Trajectory(prs) and Primitive::max_vel / max_acc / max_jrk, validate_primitive on the
 * device.  Exported by libmplx.so next to include/mplx.h, whose ABI version it does not change.
 *
 * Reference: include/mpl_basis/primitive.h:152-193 (extrema_v / _a / _j), 309-313 (the constructor from coefficients),
 * 353-394 (max_vel / max_acc / max_jrk), 450-496 (validate_primitive, validate_xxx); include/mpl_basis/math.h:21-66,
 * 117-131 (quad, cubic, solve).
 *
 * mplx_poly_load fills a poly from segments instead of a solve.  Everything is problem-minor.  Problem k has
 * S_k = n_segs[k] segments (NULL: w_max - 1 each; values above w_max - 1 count as w_max - 1), segment s has the duration
 * dts[s * dt_stride + k] and, for axis a = 0 .. D-1 and a = D (the yaw primitive), the coefficients c(0) .. c(5) of
 * primitive.h:128-131 at coeff[((s * (D + 1) + a) * 6 + j) * coeff_stride + k].  Of the yaw primitive c(4) (the rate) and
 * c(5) are kept: the yaw primitives of this library are linear, as the reference's.  taus[0] = 0, taus[s+1] = taus[s] +
 * dts[s] by sequential addition, T = taus[S].  The waypoints of the set (mplx_poly_info's seg_state) are evaluated:
 * waypoint s is segment s at 0.0, the last one the last segment at its duration, field t = taus[s].  `control` is any of
 * the eight flags; a poly remembers the control of its last solve or load.  Afterwards mplx_poly_info / _sample /
 * _traverse run on the loaded set as on a solved one.
 *
 * Status of a loaded problem: MPLX_SOLVE_EMPTY for S_k < 1, MPLX_SOLVE_BAD_TIME for a duration that is not finite or
 * <= 0.  A problem with a status bit writes its status only.
 *
 * mplx_poly_limits: per trajectory and axis the maximum over its segments of Primitive::max_vel / max_acc / max_jrk
 * ([D][max_stride]), exceed (bit 0 / 1 / 2: the largest axis maximum of vel / acc / jrk is > mv / ma / mj; never for a
 * limit <= 0, which means "not checked", primitive.h:485), valid (the AND over the segments of validate_primitive(seg,
 * mv, ma, mj, 0) under the set's control: ACC checks vel, JRK vel and acc, SNP all three, VEL nothing; the yaw bit adds
 * nothing since myaw = 0) and first_bad (the first segment that fails, else -1).  Problems with a solve or load status
 * are skipped: their outputs keep the caller's bytes.
 *
 *   MPLX_LIMITS_REFERENCE: the reference expression for expression, quirks included: of the roots solve() returns, in
 *     its order, `0 < r < t` is taken, `r >= t` ENDS the scan, anything else (negative, NaN) is passed over.  quad and the
 *     acos branch of cubic return their largest root first, so smaller roots inside (0, t) are often never looked at
 *     and the maximum is under-reported -- as the reference under-reports it.
 *   MPLX_LIMITS_ALL_ROOTS: the same roots, every one of them considered, and the acos argument clamped to [-1, 1]: the
 *     maximum of |x| over [0, t] up to the rounding of the formulas; it never over-reports.  One root is added: the
 *     reference's extrema_j returns -c1 * 2 / c0, twice the time at which the jerk's derivative c0 t + c1 vanishes
 *     (primitive.h:189), so its max_jrk misses the peak of a jerk parabola; this mode also looks at -c1 / c0.
 *
 * The branch decisions are IEEE arithmetic (-ffp-contract=off); cbrt, acos and cos are the device library's.  The
 * result is a pure function of the inputs: per-segment maxima, then one ordered pass per trajectory.
 *
 * The _device forms are asynchronous on the context's stream with no host read; the host-pointer twins stage through
 * the context's arena and are synchronous.  Every output pointer is optional.
 *
 * Errors: MPLX_ERR_ARG for NULL poly / in / out, NULL coeff or dts with n_prob > 0 (without src), a src of another
 * context, of another dimension's table or never filled, src == poly, strides below n_prob, w_max < 2 or
 * above the poly's, n_prob above k_cap, a control that is none of the eight flags, a mode other than the two;
 * MPLX_ERR_STATE for limits before any solve or load.  n_prob == 0 is a successful no-op. */
#ifndef MPLX_LIMITS_H
#define MPLX_LIMITS_H

#include "mplx_solve.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_LIMITS_REFERENCE = 0, MPLX_LIMITS_ALL_ROOTS = 1 };
enum { MPLX_EXCEED_VEL = 1, MPLX_EXCEED_ACC = 2, MPLX_EXCEED_JRK = 4 };

typedef struct {
  int64_t n_prob;          /* K                                                                                          */
  int32_t w_max;           /* segments per problem + 1                                                                   */
  int32_t control;         /* any of MPLX_VEL / ACC / JRK / SNP, with or without the yaw bit                             */
  const int32_t *n_segs;   /* [K] S_k, or NULL: w_max - 1 each                                                           */
  const double *dts;       /* [w_max - 1][dt_stride]                                                                     */
  int64_t dt_stride;
  const double *coeff;     /* [w_max - 1][D + 1][6][coeff_stride]                                                        */
  int64_t coeff_stride;
  /* the gather form (dts and coeff are then not read): segment s of problem k is the single segment of problem
     src_index[s * index_stride + k] of `src` -- coefficients, yaw primitive and duration, bit for bit; -1 ends the
     trajectory (n_segs is not read); an index outside the set src holds, or a src problem without a segment, is
     MPLX_SOLVE_EMPTY */
  mplx_poly *src;
  const int32_t *src_index;  /* [w_max - 1][index_stride], device memory in both forms of the call                       */
  int64_t index_stride;
} mplx_poly_load_in;

typedef struct {
  uint8_t *status;         /* [K]                                                                                        */
  int32_t *n_segs;         /* [K] S_k                                                                                    */
  double *total_time;      /* [K] T                                                                                      */
  double *taus;            /* [w_max][taus_stride]: taus[0 .. S_k]                                                       */
  int64_t taus_stride;
} mplx_poly_load_out;

int mplx_poly_load_device(mplx_poly *poly, const mplx_poly_load_in *d_in, const mplx_poly_load_out *d_out);
int mplx_poly_load(mplx_poly *poly, const mplx_poly_load_in *h_in, const mplx_poly_load_out *h_out);

typedef struct {
  double mv, ma, mj;       /* <= 0: not checked                                                                          */
  int32_t mode;            /* MPLX_LIMITS_REFERENCE / MPLX_LIMITS_ALL_ROOTS                                              */
} mplx_limits_in;

typedef struct {
  double *max_vel, *max_acc, *max_jrk;  /* [D][max_stride] each                                                          */
  int64_t max_stride;
  uint8_t *exceed;         /* [K] MPLX_EXCEED_* bits                                                                     */
  uint8_t *valid;          /* [K] 1 / 0                                                                                  */
  int32_t *first_bad;      /* [K] segment, or -1                                                                         */
} mplx_limits_out;

int mplx_poly_limits_device(mplx_poly *poly, const mplx_limits_in *in, const mplx_limits_out *d_out);
int mplx_poly_limits(mplx_poly *poly, const mplx_limits_in *in, const mplx_limits_out *h_out);

/* Shortcutting a chain of states (a search path: short constant-control pieces) by two-point primitives.  For every
 * query k and every pair i < j <= i + max_hop of its chain states the primitive from state i to state j with duration
 * t_j - t_i (one IEEE subtraction of the states' t rows) is solved -- every derivative up to the control's order fixed at
 * both ends, the yaw ends as they are --, its efforts, limits (MPLX_LIMITS_ALL_ROOTS with the context's v_max, a_max,
 * j_max) and traversal (the context's map, v_max, res) are evaluated, and a dynamic programme per query picks the
 * cheapest chain of hops from state 0 to state W_k - 1:
 *   edge cost c[i][j] = (J + w T) + trav: J the effort row of the control's own order, w the context's time weight;
 *   a non-adjacent edge is admitted iff its solve status is 0, it is valid and trav is finite; the adjacent edge
 *   (j = i + 1) is always admitted, a trav that is not finite counting as 0.0 (the search validated it by its own
 *   sampling); an adjacent edge with a solve status (e.g. t_{i+1} <= t_i) makes the query MPLX_SHORTCUT_BAD_CHAIN: the
 *   identity chain, costs NaN;
 *   dist[0] = 0.0, dist[j] = min over max(0, j - max_hop) <= i < j of dist[i] + c[i][j], one add per candidate, ties to
 *   the smallest i; cost = dist[W - 1]; chain_cost = the sequential sum of the adjacent edges' costs.
 * Pair p = (k (w_max - 1) + i) max_hop + (j - i - 1); pairs with j >= W_k are empty problems.  `pairs` (k_cap >=
 * Q (w_max - 1) max_hop, w_max >= 2) holds the pair set afterwards, `result` (k_cap >= Q, the chain's w_max) the Q chosen
 * trajectories, gathered from the pairs without a second solve.  W_k < 2 is MPLX_SOLVE_EMPTY.  A MPLX_SHORTCUT_BAD_CHAIN
 * query has no trajectory either: its identity chain holds the pair whose solve failed, which has no segment to gather,
 * so its problem of `result` is MPLX_SOLVE_EMPTY (no segments, no samples), as that of an empty query.  All launches
 * are queued on the context's stream with no read-back between them.  states / n_wp / every output: device memory
 * (_device) or host memory (the twin, synchronous); every output is optional.  Errors: MPLX_ERR_ARG for NULLs, polys of
 * two contexts or too small, max_hop < 1, a stride below Q, a control other than VEL / ACC / JRK; MPLX_ERR_STATE without a
 * map or with v_max <= 0. */
enum { MPLX_SHORTCUT_BAD_CHAIN = 16 };

typedef struct {
  const double *states;    /* field f of state w of query k at states[(f * w_max + w) * stride + k]: mplx_traj_info's
                              seg_state layout                                                                           */
  int64_t n_query;         /* Q                                                                                          */
  int32_t w_max;
  int32_t control;         /* MPLX_VEL / ACC / JRK, with or without the yaw bit                                          */
  int64_t stride;
  const int32_t *n_wp;     /* [Q] W_k, or NULL: w_max each; a count above w_max behaves as w_max                         */
  int32_t max_hop;         /* >= 1                                                                                       */
} mplx_shortcut_in;

typedef struct {
  uint8_t *status;         /* [Q] 0, MPLX_SOLVE_EMPTY or MPLX_SHORTCUT_BAD_CHAIN                                         */
  int32_t *n_keep;         /* [Q] kept states                                                                            */
  int32_t *keep;           /* [w_max][keep_stride] ascending state indices 0 .. W_k - 1; rows past n_keep are -1         */
  int64_t keep_stride;
  double *cost, *chain_cost;  /* [Q]                                                                                     */
  double *edge_cost;       /* [Q (w_max - 1) max_hop] c of every pair; +inf where the edge is not admitted               */
  const mplx_solve_out *pair_out;  /* device rows for the pair solve (e.g. its coefficients), or NULL; _device form only */
} mplx_shortcut_out;

int mplx_shortcut_device(mplx_poly *pairs, mplx_poly *result, const mplx_shortcut_in *d_in, const mplx_shortcut_out *d_out);
int mplx_shortcut(mplx_poly *pairs, mplx_poly *result, const mplx_shortcut_in *h_in, const mplx_shortcut_out *h_out);

#ifdef __cplusplus
}
#endif
#endif
