/* mplx_conflict.h -- conflicts between the K trajectories of one set on a common clock: which robots come closer than
 * the sum of their radii, when first, with whom, and how close they ever get.  Exported by libmplx.so next to
 * include/mplx.h, whose ABI version it does not change.  The reference has nothing of the kind; what is normative is
 * stated here and restated sequentially in tests/conflict_model.py.
 *
 * The set is either the one an mplx_poly holds (solved, loaded, scaled: mplx_poly_conflicts) or K action chains on a
 * context (mplx_traj_conflicts: the chain launch of include/mplx_traj.h runs first).  No map is needed.
 *
 * All arithmetic is IEEE double under -ffp-contract=off, in the order written.
 *
 *   Time.      Instant i, 0 <= i < n_steps, is at t_i = (double)i * step.  The local time of trajectory k is
 *              tl = t_i - t0[k] (tl = t_i without t0).  t0 may be negative.
 *   Position.  The pos rows mplx_poly_sample / mplx_traj_sample write in MPLX_TRAJ_COMMAND form for the time tl: the same
 *              clamp to [0, total], the same segment look-up and, on a poly that holds a Lambda, the same getTau under
 *              the Lambda's mode (the kernels call the device functions the samplers call).  A tl that is not finite
 *              gives a NaN position, as it does there.
 *   Active.    MPLX_CONFLICT_PARK: at every instant -- the robot waits at its start before t0 and at its end afterwards.
 *              MPLX_CONFLICT_GONE: only where tl >= 0 && tl <= total, total being the scaled total where the problem
 *              holds a Lambda.
 *   Excluded.  A trajectory with a solve / load / trajectory status (any bit, or S == 0) is excluded; so is one whose t0
 *              is not finite or whose radius is negative or not finite: that one gets MPLX_CONFLICT_BAD_INPUT in its
 *              status.  An excluded trajectory never conflicts with anything; its outputs are -1, -1, +inf.
 *   Pair test. For a != b, both included, group[a] != group[b] (without `group` every trajectory is its own group) and
 *              both active at i:  d2 = ((dx * dx) + dy * dy) + dz * dz  in axis order (two terms in 2-D), with
 *              dx = pos_a[0] - pos_b[0] ..., rr = r[a] + r[b]; a conflict iff d2 < rr * rr.  Strict: touching is none.  A
 *              d2 that is NaN is neither a conflict nor a candidate for the minimum.  (d2 and rr are symmetric in a, b:
 *              x * x == (-x) * (-x) and IEEE addition commutes.)
 *   Charging.  Without `rank` a pair is charged to both trajectories.  With it the pair is charged to a iff
 *              rank[b] <= rank[a]: the lower priority (larger rank) yields, equal ranks both do.
 *
 * Outputs, per trajectory, over the pairs charged to it:
 *   first_step     the smallest i with a conflict, else -1
 *   first_partner  the smallest index among the partners it conflicts with at that instant, else -1
 *   min_d2         the smallest d2 over the instants where both are active (conflict or not); +inf if there is none
 *   status         the set's status bits | MPLX_CONFLICT_BAD_INPUT
 * and pair_first[a * pair_stride + b]: the first instant at which a and b conflict REGARDLESS of rank -- symmetric, -1 on
 * the diagonal, for excluded trajectories, for one group and for pairs that never conflict.  Entries past K (and the
 * columns past K of a row) keep the caller's bytes.  Every output pointer is optional.
 *
 * chunk_steps: the instants processed per pass; 0 is automatic (the position table of a pass stays under
 * MPLX_CONFLICT_SCRATCH_BYTES however large n_steps is, one instant at the least).  Like `lanes` of a traversal, no
 * result depends on it: every result is a minimum -- of (i << 32 | partner), of the bit pattern of d2 (non-negative
 * doubles order like uint64), of i -- and so a pure function of the inputs whatever the tiling and the chunking.
 *
 * The _device forms are asynchronous on the context's stream with no host read; the host-pointer twins stage through
 * the context's arena and are synchronous.
 *
 * Errors: MPLX_ERR_ARG for a NULL poly / context / set / in / out, a step that is not finite or <= 0, n_steps < 1, a
 * mode other than the two, chunk_steps < 0, pair_first with pair_stride < K, and what include/mplx_traj.h says of a
 * set; MPLX_ERR_STATE before any solve or load (poly) or without params / controls (chains).  K == 0 is a no-op. */
#ifndef MPLX_CONFLICT_H
#define MPLX_CONFLICT_H

#include "mplx_scale.h"
#include "mplx_traj.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { MPLX_CONFLICT_PARK = 0, MPLX_CONFLICT_GONE = 1 };
/* clear of MPLX_TRAJ_* (1, 2, 4), MPLX_SOLVE_* (1, 2, 8), MPLX_SHORTCUT_BAD_CHAIN (16) and MPLX_LAMBDA_* (32, 64) */
enum { MPLX_CONFLICT_BAD_INPUT = 128 };
enum { MPLX_CONFLICT_SCRATCH_BYTES = 32 << 20 };

typedef struct {
  double step;            /* > 0 and finite                                                    */
  int32_t n_steps;        /* >= 1                                                              */
  int32_t mode;           /* MPLX_CONFLICT_PARK or MPLX_CONFLICT_GONE                          */
  const double *t0;       /* [K] or NULL: 0 each                                               */
  const double *radius;   /* [K] or NULL: radius_all each                                      */
  double radius_all;
  const int32_t *group;   /* [K] or NULL: every trajectory its own group                       */
  const int32_t *rank;    /* [K] or NULL: every pair is charged to both                        */
  int32_t chunk_steps;    /* 0: automatic                                                      */
} mplx_conflict_in;

typedef struct {
  int32_t *first_step;    /* [K]                                                               */
  int32_t *first_partner; /* [K]                                                               */
  double *min_d2;         /* [K]                                                               */
  uint8_t *status;        /* [K]                                                               */
  int32_t *pair_first;    /* [K][pair_stride] or NULL                                          */
  int64_t pair_stride;    /* >= K where pair_first is given                                    */
} mplx_conflict_out;

int mplx_poly_conflicts_device(mplx_poly *poly, const mplx_conflict_in *d_in, const mplx_conflict_out *d_out);
int mplx_poly_conflicts(mplx_poly *poly, const mplx_conflict_in *h_in, const mplx_conflict_out *h_out);
int mplx_traj_conflicts_device(mplx_ctx *ctx, const mplx_traj_set *d_set, const mplx_conflict_in *d_in,
                               const mplx_conflict_out *d_out);
int mplx_traj_conflicts(mplx_ctx *ctx, const mplx_traj_set *h_set, const mplx_conflict_in *h_in, const mplx_conflict_out *h_out);

#ifdef __cplusplus
}
#endif
#endif
