// rollout_api.cpp -- C ABI of include/mplx_rollout.h: batched rollouts on the map the context holds
// (rollout_kernel.hip).  mplx_rollout_device is one asynchronous launch; mplx_rollout stages host arrays, runs the same
// launch and resolves the rollouts that met a heading-limit decision inside the band of the yaw pinning by stepping
// them through the pinned dense expansion (mplx_expand).
#include "mplx_ctx.h"
#include "../../include/mplx_rollout.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

using namespace mplx_detail;

namespace {

int check_args(mplx_ctx *c, const char *who, const void *starts, int64_t n_starts, int64_t start_stride, const void *actions,
               int64_t n, int32_t horizon, int64_t action_stride, const mplx_rollout_out *o) {
  if (!o || horizon < 1 || n < 0 || (n_starts != 1 && n_starts != n) || start_stride < n_starts || action_stride < n ||
      (n > 0 && (!starts || !actions)) || (o->end_state && o->end_stride < n))
    return fail(c, MPLX_ERR_ARG, "%s: bad arguments", who);
  if (int rc = ctx_ready(c)) return rc;
  if ((o->end_heur || o->end_flags) && !c->has_goal)
    return fail(c, MPLX_ERR_STATE, "%s: end_heur / end_flags need mplx_set_goal", who);
  return MPLX_OK;
}

// One launch on device pointers; the arguments have been checked.
int launch(mplx_ctx *c, const double *d_starts, int64_t n_starts, int64_t start_stride, const int32_t *d_actions, int64_t n,
           int32_t horizon, int64_t action_stride, const mplx_rollout_out *o) {
  const mplx_succ none{};
  mplx::RolloutArgs a{};
  a.env = expand_args(c, nullptr, 0, 0, &none);
  // the band of the yaw pinning (margin, the exact-tie exemption); nothing is recorded per node and nothing becomes
  // pending: a rollout carries its own flag
  if (int rc = yaw_slot(c, &a.env.yaw)) return rc;
  a.band = a.env.yaw.amb ? 1 : 0;
  a.env.yaw.amb = nullptr;
  a.env.yaw.any_host = nullptr;
  a.starts = d_starts; a.n_starts = n_starts; a.start_stride = start_stride;
  a.actions = d_actions; a.n_rollouts = n; a.action_stride = action_stride; a.horizon = horizon;
  a.u_lds = (size_t)c->nU * c->udim * sizeof(double) <= mplx::kRolloutLdsControls ? 1 : 0;
  a.status = o->status; a.steps = o->steps; a.cost = o->cost; a.prefix_cost = o->prefix_cost;
  a.end_state = o->end_state; a.end_stride = o->end_stride; a.end_hash = o->end_hash;
  a.post = c->goal_fuse;
  a.post.heur = o->end_heur;
  a.post.flags = o->end_flags;
  HIP_TRY(c, mplx::launch_rollout(c->dim, c->prm.control, a, c->stream));
  return MPLX_OK;
}

// end_heur / end_flags of one end state on the host: env_base.h:46-64 (default branch) and env_map.h:25-37 as
// mplx_device_common.h post_eval states them (comparisons, one product and one quotient: the same bits on either side).
void host_post(const mplx::PostFuse &P, int D, uint64_t hash, const double *s, int64_t stride, double *heur, uint8_t *flags) {
  auto linf = [&](int lo) {
    double m = 0;
    for (int i = 0; i < D; i++) {
      const double d = std::fabs(s[(int64_t)(lo + i) * stride] - P.goal[lo + i]);
      m = d > m ? d : m;
    }
    return m;
  };
  const bool is_goal_state = hash == P.goal_hash;
  const double m = linf(0);
  if (heur) *heur = is_goal_state ? 0.0 : (P.v_max > 0 ? P.w * m / P.v_max : P.w * m);
  bool goaled = m <= P.tol_pos;
  if (goaled && P.tol_vel >= 0) goaled = linf(D) <= P.tol_vel;
  if (goaled && P.tol_acc >= 0) goaled = linf(2 * D) <= P.tol_acc;
  if (goaled && P.tol_yaw >= 0) goaled = std::fabs(s[(int64_t)(4 * D) * stride] - P.goal[4 * D]) <= P.tol_yaw;
  if (flags) *flags = (uint8_t)((goaled ? 1u : 0u) | (is_goal_state ? 2u : 0u));
}

}  // namespace

extern "C" {

int mplx_rollout_device(mplx_ctx *c, const double *d_starts, int64_t n_starts, int64_t start_stride, const int32_t *d_actions,
                        int64_t n_rollouts, int32_t horizon, int64_t action_stride, const mplx_rollout_out *d_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_args(c, "mplx_rollout_device", d_starts, n_starts, start_stride, d_actions, n_rollouts, horizon,
                          action_stride, d_out))
    return rc;
  if (n_rollouts == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  return launch(c, d_starts, n_starts, start_stride, d_actions, n_rollouts, horizon, action_stride, d_out);
}

int mplx_rollout(mplx_ctx *c, const double *h_starts, int64_t n_starts, int64_t start_stride, const int32_t *h_actions,
                 int64_t n_rollouts, int32_t horizon, int64_t action_stride, const mplx_rollout_out *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_args(c, "mplx_rollout", h_starts, n_starts, start_stride, h_actions, n_rollouts, horizon, action_stride,
                          h_out))
    return rc;
  if (n_rollouts == 0) return MPLX_OK;
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const int D = c->dim, F = 4 * D + 2, nU = c->nU;
  const int64_t n = n_rollouts, H = horizon;
  const bool yaw_limit = (c->prm.control & 0x10) && c->prm.yaw_max > 0;
  // One arena block: starts [F][n_starts], actions [H][n], then the output rows.  The status, steps, prefix, end state
  // and end hash rows are always produced: resolving a rollout inside the band needs them.
  const size_t N = (size_t)n;
  StageLayout l;
  const size_t o_starts = l.add((size_t)F * n_starts * 8), o_actions = l.add((size_t)H * N * 4), o_status = l.add(N),
               o_steps = l.add(N * 4), o_cost = l.add(N * 8), o_prefix = l.add(N * 8), o_state = l.add((size_t)F * N * 8),
               o_hash = l.add(N * 8), o_heur = l.add(h_out->end_heur ? N * 8 : 0), o_flags = l.add(h_out->end_flags ? N : 0);
  if (int rc = stage_commit(c, &l)) return rc;
  HIP_TRY(c, stage_in_rows(c, l.base + o_starts, h_starts, (size_t)start_stride * 8, (size_t)n_starts * 8, F));
  HIP_TRY(c, stage_in_rows(c, l.base + o_actions, h_actions, (size_t)action_stride * 4, N * 4, H));
  mplx_rollout_out d{};
  d.status = (uint8_t *)(l.base + o_status);
  d.steps = (int32_t *)(l.base + o_steps);
  d.cost = (double *)(l.base + o_cost);
  d.prefix_cost = (double *)(l.base + o_prefix);
  d.end_state = (double *)(l.base + o_state);
  d.end_stride = n;
  d.end_hash = (uint64_t *)(l.base + o_hash);
  d.end_heur = h_out->end_heur ? (double *)(l.base + o_heur) : nullptr;
  d.end_flags = h_out->end_flags ? (uint8_t *)(l.base + o_flags) : nullptr;
  if (int rc = launch(c, (const double *)(l.base + o_starts), n_starts, n_starts, (const int32_t *)(l.base + o_actions), n, horizon, n,
                      &d))
    return rc;
  std::vector<uint8_t> status(N);
  HIP_TRY(c, stage_out(c, status.data(), d.status, N));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<int64_t> band;  // rollouts that met a heading-limit decision inside the band
  if (yaw_limit)
    for (int64_t k = 0; k < n; k++)
      if (status[(size_t)k] & MPLX_ROLLOUT_HEADING_BAND) band.push_back(k);

  // every row but the status to the host (a null row is skipped), then the stream is idle
  auto fetch = [&](int32_t *steps, double *cost, double *prefix, double *state, int64_t stride, uint64_t *hash, double *heur, uint8_t *flags) -> int {
    HIP_TRY(c, stage_out(c, steps, d.steps, N * 4));
    HIP_TRY(c, stage_out(c, cost, d.cost, N * 8));
    HIP_TRY(c, stage_out(c, prefix, d.prefix_cost, N * 8));
    HIP_TRY(c, stage_out_rows(c, state, (size_t)stride * 8, d.end_state, N * 8, F));
    HIP_TRY(c, stage_out(c, hash, d.end_hash, N * 8));
    HIP_TRY(c, stage_out(c, heur, d.end_heur, N * 8));
    HIP_TRY(c, stage_out(c, flags, d.end_flags, N));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MPLX_OK;
  };
  if (band.empty()) {
    if (h_out->status) std::copy(status.begin(), status.end(), h_out->status);
    return fetch(h_out->steps, h_out->cost, h_out->prefix_cost, h_out->end_state, h_out->end_stride, h_out->end_hash, h_out->end_heur,
                 h_out->end_flags);
  }

  // ---- everything to the host, then the flagged rollouts again through the pinned dense path.  Every row comes down
  // BEFORE the walk: mplx_expand below carves the same arena (rule 3 of the staging block, mplx_ctx.h).
  std::vector<int32_t> steps(N);
  std::vector<double> cost(N), prefix(N), state((size_t)F * N), heur(h_out->end_heur ? N : 0);
  std::vector<uint64_t> hash(N);
  std::vector<uint8_t> flags(h_out->end_flags ? N : 0);
  if (int rc = fetch(steps.data(), cost.data(), prefix.data(), state.data(), n, hash.data(), h_out->end_heur ? heur.data() : nullptr,
                     h_out->end_flags ? flags.data() : nullptr))
    return rc;

  // The flagged rollouts walk again from their start states, all of them one step per mplx_expand call: that call runs
  // the dense kernel with the detection and override passes of the yaw pinning, and its dense slots carry the status.
  const int64_t m = (int64_t)band.size();
  std::vector<double> cur((size_t)F * m), succ_state;
  std::vector<int64_t> live(band.size());  // positions in `band` still walking
  for (int64_t j = 0; j < m; j++) {
    live[(size_t)j] = j;
    const int64_t col = n_starts == 1 ? 0 : band[(size_t)j];
    for (int f = 0; f < F; f++) cur[(size_t)f * m + j] = h_starts[(int64_t)f * start_stride + col];
    const int64_t k = band[(size_t)j];
    status[(size_t)k] = MPLX_SLOT_FINITE;
    steps[(size_t)k] = 0;
    prefix[(size_t)k] = 0.0;
  }
  std::vector<uint8_t> had_steps(band.size(), 0);
  std::vector<double> nodes;
  std::vector<uint8_t> s_status;
  std::vector<double> s_cost;
  std::vector<uint64_t> s_hash;
  for (int64_t h = 0; h < H && !live.empty(); h++) {
    std::vector<int64_t> go;
    std::vector<int32_t> act;
    for (int64_t j : live) {
      const int64_t k = band[(size_t)j];
      const int32_t a = h_actions[h * action_stride + k];
      if (a == -1) continue;  // complete
      if (a < -1 || a >= nU) { status[(size_t)k] = MPLX_ROLLOUT_BAD_ACTION; continue; }
      go.push_back(j);
      act.push_back(a);
    }
    live.clear();
    if (go.empty()) break;
    const int64_t g = (int64_t)go.size(), slots = g * nU;
    nodes.resize((size_t)F * g);
    for (int64_t i = 0; i < g; i++)
      for (int f = 0; f < F; f++) nodes[(size_t)f * g + i] = cur[(size_t)f * m + go[(size_t)i]];
    s_status.resize((size_t)slots);
    s_cost.resize((size_t)slots);
    s_hash.resize((size_t)slots);
    succ_state.resize((size_t)F * slots);
    mplx_succ so{};
    so.status = s_status.data();
    so.cost = s_cost.data();
    so.hash = s_hash.data();
    so.state = succ_state.data();
    so.state_stride = slots;
    if (int rc = mplx_expand(c, nodes.data(), g, g, &so)) return rc;
    for (int64_t i = 0; i < g; i++) {
      const int64_t j = go[(size_t)i], k = band[(size_t)j], slot = i * nU + act[(size_t)i];
      const uint8_t st = s_status[(size_t)slot];
      if (st != MPLX_SLOT_FINITE) { status[(size_t)k] = st; continue; }
      prefix[(size_t)k] = prefix[(size_t)k] + s_cost[(size_t)slot];
      steps[(size_t)k] += 1;
      for (int f = 0; f < F; f++) cur[(size_t)f * m + j] = succ_state[(size_t)f * slots + slot];
      hash[(size_t)k] = s_hash[(size_t)slot];
      had_steps[(size_t)j] = 1;
      live.push_back(j);
    }
  }
  // A flagged rollout without a step under the pinned decisions needs the hash of its START state, and the launch
  // wrote the hash of whatever end state device trig reached: one more launch of horizon 1 with the action -1 hashes
  // the start states (no pair is evaluated).
  std::vector<int64_t> rehash;
  for (int64_t j = 0; j < m; j++)
    if (!had_steps[(size_t)j]) rehash.push_back(j);
  if (!rehash.empty()) {
    const int64_t r = (int64_t)rehash.size();
    std::vector<double> st0((size_t)F * r);
    std::vector<int32_t> minus1((size_t)r, -1);
    for (int64_t i = 0; i < r; i++)
      for (int f = 0; f < F; f++) st0[(size_t)f * r + i] = cur[(size_t)f * m + rehash[(size_t)i]];
    StageRows sr;  // (the arena again: nothing of the first launch is still needed on the device)
    const auto i_st0 = sr.in(st0.data(), st0.size() * 8), i_minus1 = sr.in(minus1.data(), (size_t)r * 4), o_h0 = sr.landed((size_t)r * 8);
    if (int rc = stage_commit(c, &sr)) return rc;
    mplx_rollout_out ho{};
    ho.end_hash = sr.dev<uint64_t>(o_h0);
    if (int rc = launch(c, sr.dev<double>(i_st0), r, r, sr.dev<int32_t>(i_minus1), r, 1, r, &ho)) return rc;
    if (int rc = stage_fetch(c, &sr)) return rc;
    const uint64_t *h0 = sr.host<uint64_t>(o_h0);
    for (int64_t i = 0; i < r; i++) hash[(size_t)band[(size_t)rehash[(size_t)i]]] = h0[(size_t)i];
  }
  for (int64_t j = 0; j < m; j++) {
    const int64_t k = band[(size_t)j];
    cost[(size_t)k] = status[(size_t)k] == MPLX_SLOT_FINITE ? prefix[(size_t)k] : std::numeric_limits<double>::infinity();
    for (int f = 0; f < F; f++) state[(size_t)f * n + k] = cur[(size_t)f * m + j];
    if (h_out->end_heur || h_out->end_flags)
      host_post(c->goal_fuse, D, hash[(size_t)k], &state[(size_t)k], n, h_out->end_heur ? &heur[(size_t)k] : nullptr,
                h_out->end_flags ? &flags[(size_t)k] : nullptr);
  }
  for (int64_t k = 0; k < n; k++) status[(size_t)k] &= (uint8_t)~MPLX_ROLLOUT_HEADING_BAND;
  if (h_out->status) std::copy(status.begin(), status.end(), h_out->status);
  if (h_out->steps) std::copy(steps.begin(), steps.end(), h_out->steps);
  if (h_out->cost) std::copy(cost.begin(), cost.end(), h_out->cost);
  if (h_out->prefix_cost) std::copy(prefix.begin(), prefix.end(), h_out->prefix_cost);
  if (h_out->end_state)
    for (int f = 0; f < F; f++)
      std::copy(state.begin() + (size_t)f * n, state.begin() + (size_t)(f + 1) * n, h_out->end_state + (int64_t)f * h_out->end_stride);
  if (h_out->end_hash) std::copy(hash.begin(), hash.end(), h_out->end_hash);
  if (h_out->end_heur) std::copy(heur.begin(), heur.end(), h_out->end_heur);
  if (h_out->end_flags) std::copy(flags.begin(), flags.end(), h_out->end_flags);
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

}  // extern "C"
