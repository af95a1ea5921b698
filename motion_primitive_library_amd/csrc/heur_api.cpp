// heur_api.cpp -- C ABI of include/mplx_heur.h for batches of states: mplx_heur_eval_device on resident rows
// (heur_kernel.hip) and its host-pointer twin, which copies the rows through a block of its own (the shared staging arena
// belongs to the entry points the staging walks of tests/test_gpu_staging_*.py cover).  The
// open set's mode is open_api.cpp's, the host planner's planner_capi.cpp's.
#include "mplx_ctx.h"
#include "../../include/mplx_heur.h"

using namespace mplx_detail;

namespace {

int heur_args(mplx_ctx *c, const char *who, const mplx_goal_spec *goal, int32_t mode, const double *states, int64_t K, int64_t stride,
              double *out, mplx::HeurArgs *a) {
  if (!goal || K < 0 || stride < K || (K > 0 && (!states || !out))) return fail(c, MPLX_ERR_ARG, "%s: NULL goal / states / out, K < 0 or stride < K", who);
  if (mode == MPLX_HEUR_REFERENCE)
    return fail(c, MPLX_ERR_ARG, "%s: MPLX_HEUR_REFERENCE is host only (the planner's mode): the device takes DEFAULT and ROBUST", who);
  if (mode != MPLX_HEUR_DEFAULT && mode != MPLX_HEUR_ROBUST) return fail(c, MPLX_ERR_ARG, "%s: unknown mode %d", who, (int)mode);
  mplx::PostFuse f{};
  if (int rc = goal_fuse_of(c, who, goal, &f)) return rc;  // NULL goal row, unknown control flags
  if (mode == MPLX_HEUR_ROBUST && !(goal->w > 0)) return fail(c, MPLX_ERR_ARG, "%s: MPLX_HEUR_ROBUST needs w > 0", who);
  a->states = states; a->n = K; a->stride = stride; a->out = out;
  for (int i = 0; i < 14; i++) a->goal[i] = f.goal[i];
  a->goal_hash = f.goal_hash;
  a->control = goal->control; a->goal_control = goal->goal_control;
  a->mode = mode;
  a->w = goal->w; a->v_max = goal->v_max;
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_heur_eval_device(mplx_ctx *c, const mplx_goal_spec *goal, int32_t mode, const double *d_states, int64_t K, int64_t stride,
                          double *d_out) {
  if (!c) return MPLX_ERR_ARG;
  mplx::HeurArgs a{};
  if (int rc = heur_args(c, "mplx_heur_eval_device", goal, mode, d_states, K, stride, d_out, &a)) return rc;
  if (K == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, mplx::launch_heur_eval(c->dim, a, c->stream));
  return MPLX_OK;
}

int mplx_heur_eval(mplx_ctx *c, const mplx_goal_spec *goal, int32_t mode, const double *h_states, int64_t K, int64_t stride, double *h_out) {
  if (!c) return MPLX_ERR_ARG;
  mplx::HeurArgs a{};
  if (int rc = heur_args(c, "mplx_heur_eval", goal, mode, h_states, K, stride, h_out, &a)) return rc;
  if (K == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  // the rows go through a block of the call's own (c->heur_ws), carved like an arena row but not part of the shared arena:
  // no other entry point holds rows in it, and the call synchronises before it returns
  const size_t n = (size_t)K, F = 4 * (size_t)c->dim + 2;
  StageLayout l;
  const size_t i_s = l.add(F * n * 8), o_h = l.add(n * 8);
  if (int rc = ensure(c, c->heur_ws, l.total)) return rc;
  l.base = (char *)c->heur_ws.p;
  HIP_TRY(c, stage_in_rows(c, l.base + i_s, h_states, (size_t)stride * 8, n * 8, F));
  a.states = (const double *)(l.base + i_s);
  a.stride = K;
  a.out = (double *)(l.base + o_h);
  HIP_TRY(c, mplx::launch_heur_eval(c->dim, a, c->stream));
  HIP_TRY(c, stage_out(c, h_out, a.out, n * 8));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

}  // extern "C"
