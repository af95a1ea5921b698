// traj_api.cpp -- C ABI of include/mplx_traj.h: Trajectory<Dim> on the device (traj_kernel.hip).  Every call launches
// the chain kernel into the context's segment table first and its own kernel after it on the same stream; the
// host-pointer twins stage through the context's arena and scatter the compact device rows into the caller's strides.
#include "mplx_ctx.h"
#include "../../include/mplx_traj.h"

#include <algorithm>
#include <cmath>

using namespace mplx_detail;

namespace {

int check_set(mplx_ctx *c, const char *who, const mplx_traj_set *s, const void *out) {
  if (!s || !out || s->horizon < 1 || s->n_traj < 0 || (s->n_starts != 1 && s->n_starts != s->n_traj) ||
      s->start_stride < s->n_starts || s->action_stride < s->n_traj || (s->n_traj > 0 && (!s->starts || !s->actions)))
    return fail(c, MPLX_ERR_ARG, "%s: bad arguments", who);
  if (!c->has_params) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_params has not been called", who);
  if (!c->has_U) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_controls has not been called", who);
  const int need = c->dim + ((c->prm.control & 0x10) ? 1 : 0);
  if (c->udim < need) return fail(c, MPLX_ERR_STATE, "%s: controls have %d entries per row, the control flag needs %d", who, c->udim, need);
  return MPLX_OK;
}

int check_times(mplx_ctx *c, const char *who, const mplx_traj_set *s, const mplx_traj_times *t, const mplx_traj_sample_out *o,
                int64_t *count) {
  if (!t || (t->form != MPLX_TRAJ_COMMAND && t->form != MPLX_TRAJ_WAYPOINT) || t->n_uniform < 0 ||
      (t->n_uniform == 0 && (t->n_times < 1 || t->time_stride < 0 || (t->time_stride != 0 && t->time_stride < t->n_times) ||
                             (s->n_traj > 0 && !t->times))))
    return fail(c, MPLX_ERR_ARG, "%s: bad times (N >= 1, or Q >= 1 values with a stride of 0 or >= Q) or form", who);
  *count = t->n_uniform > 0 ? (int64_t)t->n_uniform + 1 : t->n_times;
  if (o->out && (o->sample_stride < *count || o->row_stride / o->sample_stride < s->n_traj))
    return fail(c, MPLX_ERR_ARG, "%s: sample_stride < samples or row_stride < n_traj * sample_stride", who);
  return MPLX_OK;
}

int check_traverse(mplx_ctx *c, const char *who, int32_t lanes) {
  if (lanes != 0 && lanes != 4 && lanes != 16 && lanes != 64) return fail(c, MPLX_ERR_ARG, "%s: lanes must be 0, 4, 16 or 64", who);
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "%s: set the map first", who);
  if (c->n_cells > 0x7fffffffLL) return fail(c, MPLX_ERR_STATE, "%s: the map has more cells than getIndex (int32) can number", who);
  if (!(c->prm.v_max > 0)) return fail(c, MPLX_ERR_STATE, "%s: v_max must be > 0 (env_map.h:231)", who);
  return MPLX_OK;
}

// The segment table of `s` in the context's scratch and the chain launch that fills it (+ the info rows of `io`).
int build(mplx_ctx *c, const mplx_traj_set *s, const mplx_traj_info_out *io, mplx::TrajArgs *out) {
  const mplx_succ none{};
  mplx::TrajArgs a{};
  a.env = expand_args(c, nullptr, 0, 0, &none);
  a.starts = s->starts; a.n_starts = s->n_starts; a.start_stride = s->start_stride;
  a.actions = s->actions; a.n_traj = s->n_traj; a.action_stride = s->action_stride; a.horizon = s->horizon;
  a.yaw = (c->prm.control & 0x10) ? 1 : 0;
  const size_t N = (size_t)s->n_traj, H = (size_t)s->horizon, NC = 5 * (size_t)c->dim + 2;
  StageLayout l;  // (only the carving: the table is the context's own scratch, not the arena)
  const size_t o_S = l.add(N * 4), o_n = l.add(N * 4), o_st = l.add(N), o_T = l.add(N * 8), o_tau = l.add((H + 1) * N * 8), o_seg = l.add(H * NC * N * 8);
  if (int rc = ensure(c, c->traj_tab, l.total)) return rc;
  char *base = (char *)c->traj_tab.p;
  a.tab_S = (int32_t *)(base + o_S);
  a.tab_n = (int32_t *)(base + o_n);
  a.tab_status = (uint8_t *)(base + o_st);
  a.tab_T = (double *)(base + o_T);
  a.tab_tau = (double *)(base + o_tau);
  a.tab_seg = (double *)(base + o_seg);
  if (io) {
    a.status = io->status; a.n_segs = io->n_segs; a.total_time = io->total_time;
    a.effort = io->effort; a.effort_stride = io->effort_stride;
    a.seg_state = io->seg_state; a.seg_stride = io->seg_stride;
  }
  HIP_TRY(c, mplx::launch_traj_chain(c->dim, c->prm.control, a, c->stream));
  *out = a;
  return MPLX_OK;
}

int check_info(mplx_ctx *c, const char *who, const mplx_traj_set *s, const mplx_traj_info_out *o) {
  if ((o->effort && o->effort_stride < s->n_traj) || (o->seg_state && o->seg_stride < s->n_traj))
    return fail(c, MPLX_ERR_ARG, "%s: effort_stride / seg_stride < n_traj", who);
  return MPLX_OK;
}

// n_segs: the segment counts as well (the host twin needs them: they decide which samples exist)
int sample_launch(mplx_ctx *c, const mplx_traj_set *s, const mplx_traj_times *t, const mplx_traj_sample_out *o, int64_t count, int32_t *n_segs = nullptr) {
  mplx_traj_info_out io{};
  io.status = o->status;
  io.n_segs = n_segs;
  mplx::TrajArgs a;
  if (int rc = build(c, s, &io, &a)) return rc;
  if (!o->out) return MPLX_OK;
  a.n_uniform = t->n_uniform; a.times = t->times; a.time_stride = t->n_uniform > 0 ? 0 : t->time_stride; a.count = count;
  a.out = o->out; a.row_stride = o->row_stride; a.sample_stride = o->sample_stride;
  HIP_TRY(c, mplx::launch_traj_sample(c->dim, t->form, a, c->stream));
  return MPLX_OK;
}

// Lanes per trajectory from the bound B = ceil(v_max horizon dt / res) + 1 on the samples, known without reading device
// data: the smallest G of {4, 16, 64} with ceil(B / G) <= 16 rounds.  (The ray call's 4 rounds were the starting rule;
// measured at B = 41 / 121 / 321 the fastest G is 4 / 16 / 64 -- DESIGN.md 4.9: a sample costs a segment look-up and a
// polynomial on top of its map byte, and half the trajectories end early, which wide groups cannot use.)
int auto_lanes(const mplx_ctx *c, int32_t horizon) {
  const double B = std::ceil(c->prm.v_max * (double)horizon * c->prm.dt / c->res) + 1.0;
  if (!(B > 64.0)) return 4;
  return B <= 256.0 ? 16 : 64;
}

int traverse_launch(mplx_ctx *c, const mplx_traj_set *s, int32_t lanes, const mplx_traj_traverse_out *o) {
  mplx::TrajArgs a;
  if (int rc = build(c, s, nullptr, &a)) return rc;
  a.status = o->status; a.cost = o->cost; a.n_samples = o->n_samples; a.n_cells = o->n_cells; a.stop_sample = o->stop_sample;
  HIP_TRY(c, mplx::launch_traj_traverse(c->dim, lanes ? lanes : auto_lanes(c, s->horizon), a, c->stream));
  return MPLX_OK;
}

}  // namespace

namespace mplx_detail {

int traj_check_set(mplx_ctx *c, const char *who, const mplx_traj_set *s, const void *out) { return check_set(c, who, s, out); }
int traj_build_table(mplx_ctx *c, const mplx_traj_set *s, mplx::TrajArgs *out) { return build(c, s, nullptr, out); }
// Host set -> the arena: starts [F][n_starts] and actions [H][n] packed; after the commit, the device view of the set
TrajSetRows traj_set_rows(const mplx_ctx *c, const mplx_traj_set *s, StageRows *st) {
  const size_t F = 4 * (size_t)c->dim + 2, n = (size_t)s->n_traj, ns = (size_t)s->n_starts;
  const auto starts = st->in_rows(s->starts, (size_t)s->start_stride * 8, ns * 8, F);
  return {starts, st->in_rows(s->actions, (size_t)s->action_stride * 4, n * 4, (size_t)s->horizon)};
}
mplx_traj_set traj_set_view(const mplx_traj_set *s, const StageRows &st, const TrajSetRows &r) {
  mplx_traj_set d = *s;
  d.starts = st.dev<double>(r.starts); d.start_stride = s->n_starts;
  d.actions = st.dev<int32_t>(r.actions); d.action_stride = s->n_traj;
  return d;
}

}  // namespace mplx_detail

extern "C" {

int mplx_traj_info_device(mplx_ctx *c, const mplx_traj_set *d_set, const mplx_traj_info_out *d_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_set(c, "mplx_traj_info_device", d_set, d_out)) return rc;
  if (int rc = check_info(c, "mplx_traj_info_device", d_set, d_out)) return rc;
  if (d_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  mplx::TrajArgs a;
  return build(c, d_set, d_out, &a);
}

int mplx_traj_info(mplx_ctx *c, const mplx_traj_set *h_set, const mplx_traj_info_out *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_set(c, "mplx_traj_info", h_set, h_out)) return rc;
  if (int rc = check_info(c, "mplx_traj_info", h_set, h_out)) return rc;
  if (h_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t n = (size_t)h_set->n_traj, F = 4 * (size_t)c->dim + 2, H1 = (size_t)h_set->horizon + 1;
  StageRows st;
  const TrajSetRows in = traj_set_rows(c, h_set, &st);
  const auto o_st = st.out_or_scratch(h_out->status, n), o_S = st.landed(n * 4), o_T = st.out_or_scratch(h_out->total_time, n * 8),
             o_e = st.out_rows(h_out->effort, (size_t)h_out->effort_stride * 8, n * 8, 5), o_seg = st.landed(h_out->seg_state, F * H1 * n * 8);
  if (int rc = stage_commit(c, &st)) return rc;
  const mplx_traj_set d = traj_set_view(h_set, st, in);
  mplx_traj_info_out o{};
  o.status = st.dev<uint8_t>(o_st);
  o.n_segs = st.dev<int32_t>(o_S);
  o.total_time = st.dev<double>(o_T);
  o.effort = st.dev<double>(o_e);
  o.effort_stride = (int64_t)n;
  o.seg_state = st.dev<double>(o_seg);
  o.seg_stride = (int64_t)n;
  mplx::TrajArgs a;
  if (int rc = build(c, &d, &o, &a)) return rc;
  if (int rc = stage_fetch(c, &st)) return rc;
  const int32_t *S = st.host<int32_t>(o_S);
  const double *seg = st.host<double>(o_seg);
  if (h_out->n_segs) std::copy(S, S + n, h_out->n_segs);
  if (h_out->seg_state)  // states past S_k keep the caller's bytes
    for (size_t f = 0; f < F; f++)
      for (size_t s = 0; s < H1; s++)
        for (size_t k = 0; k < n; k++)
          if ((int64_t)s <= (int64_t)S[k]) h_out->seg_state[(int64_t)(f * H1 + s) * h_out->seg_stride + (int64_t)k] = seg[(f * H1 + s) * n + k];
  return MPLX_OK;
}

int mplx_traj_sample_device(mplx_ctx *c, const mplx_traj_set *d_set, const mplx_traj_times *d_times, const mplx_traj_sample_out *d_out) {
  if (!c) return MPLX_ERR_ARG;
  int64_t count = 0;
  if (int rc = check_set(c, "mplx_traj_sample_device", d_set, d_out)) return rc;
  if (int rc = check_times(c, "mplx_traj_sample_device", d_set, d_times, d_out, &count)) return rc;
  if (d_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  return sample_launch(c, d_set, d_times, d_out, count);
}

int mplx_traj_sample(mplx_ctx *c, const mplx_traj_set *h_set, const mplx_traj_times *h_times, const mplx_traj_sample_out *h_out) {
  if (!c) return MPLX_ERR_ARG;
  int64_t count = 0;
  if (int rc = check_set(c, "mplx_traj_sample", h_set, h_out)) return rc;
  if (int rc = check_times(c, "mplx_traj_sample", h_set, h_times, h_out, &count)) return rc;
  if (h_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)h_set->n_traj, cnt = (size_t)count, D = (size_t)c->dim;
  const size_t rows = h_times->form == MPLX_TRAJ_COMMAND ? 4 * D + 3 : 4 * D + 1;
  const bool own_times = h_times->n_uniform == 0;
  const size_t n_cols = own_times ? (h_times->time_stride ? n : 1) : 0;
  const size_t src_stride = (size_t)(h_times->time_stride ? h_times->time_stride : (int64_t)cnt) * 8;
  StageRows st;
  const TrajSetRows in = traj_set_rows(c, h_set, &st);
  // the segment counts decide which samples exist: EMPTY trajectories keep the caller's bytes
  const auto i_t = st.in_rows(own_times ? h_times->times : nullptr, src_stride, cnt * 8, n_cols), o_st = st.out_or_scratch(h_out->status, n),
             o_S = st.landed(n * 4), o_out = st.landed(h_out->out, rows * n * cnt * 8);
  if (int rc = stage_commit(c, &st)) return rc;
  const mplx_traj_set d = traj_set_view(h_set, st, in);
  mplx_traj_times t = *h_times;
  if (own_times) {
    t.times = st.dev<double>(i_t);
    t.time_stride = h_times->time_stride ? (int64_t)cnt : 0;
  }
  mplx_traj_sample_out o{};
  o.out = st.dev<double>(o_out);
  o.sample_stride = (int64_t)cnt;
  o.row_stride = (int64_t)(n * cnt);
  o.status = st.dev<uint8_t>(o_st);
  if (int rc = sample_launch(c, &d, &t, &o, count, st.dev<int32_t>(o_S))) return rc;
  if (int rc = stage_fetch(c, &st)) return rc;
  const int32_t *S = st.host<int32_t>(o_S);
  const double *buf = st.host<double>(o_out);
  if (h_out->out)
    for (size_t r = 0; r < rows; r++)
      for (size_t k = 0; k < n; k++) {
        if (S[k] == 0) continue;
        std::copy(buf + (r * n + k) * cnt, buf + (r * n + k + 1) * cnt,
                  h_out->out + (int64_t)r * h_out->row_stride + (int64_t)k * h_out->sample_stride);
      }
  return MPLX_OK;
}

int mplx_traj_traverse_device(mplx_ctx *c, const mplx_traj_set *d_set, int32_t lanes, const mplx_traj_traverse_out *d_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_set(c, "mplx_traj_traverse_device", d_set, d_out)) return rc;
  if (int rc = check_traverse(c, "mplx_traj_traverse_device", lanes)) return rc;
  if (d_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  return traverse_launch(c, d_set, lanes, d_out);
}

int mplx_traj_traverse(mplx_ctx *c, const mplx_traj_set *h_set, int32_t lanes, const mplx_traj_traverse_out *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_set(c, "mplx_traj_traverse", h_set, h_out)) return rc;
  if (int rc = check_traverse(c, "mplx_traj_traverse", lanes)) return rc;
  if (h_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)h_set->n_traj;
  StageRows st;
  const TrajSetRows in = traj_set_rows(c, h_set, &st);
  const auto o_st = st.out(h_out->status, n), o_cost = st.out(h_out->cost, n * 8), o_ns = st.out(h_out->n_samples, n * 4),
             o_nc = st.out(h_out->n_cells, n * 4), o_stop = st.out(h_out->stop_sample, n * 4);
  if (int rc = stage_commit(c, &st)) return rc;
  const mplx_traj_set d = traj_set_view(h_set, st, in);
  mplx_traj_traverse_out o{};
  o.status = st.dev<uint8_t>(o_st); o.cost = st.dev<double>(o_cost); o.n_samples = st.dev<int32_t>(o_ns);
  o.n_cells = st.dev<int32_t>(o_nc); o.stop_sample = st.dev<int32_t>(o_stop);
  if (int rc = traverse_launch(c, &d, lanes, &o)) return rc;
  return stage_fetch(c, &st);
}

}  // extern "C"
