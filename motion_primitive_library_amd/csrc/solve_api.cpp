// solve_api.cpp -- C ABI of include/mplx_solve.h: the batched trajectory solver (solve_kernel.hip) and Trajectory<Dim>
// on what it returns (the POLY instantiations of traj_kernel.hip).  An mplx_poly owns the segment table of its last
// solve, laid out for the K of that solve (every array [row][K]), and the workspace of the elimination (mplx_poly.h).  The
// host-pointer twins stage through the context's arena and scatter the compact device rows into the caller's strides.
#include "mplx_poly.h"

#include <algorithm>

using namespace mplx_detail;

namespace {

int check_in(mplx_poly *p, const char *who, const mplx_solve_in *in, const mplx_solve_out *out, int *so) {
  mplx_ctx *c = p->c;
  if (!in || !out || in->n_prob < 0 || in->w_max < 2 || in->w_max > p->w_max || in->n_prob > p->k_cap)
    return fail(c, MPLX_ERR_ARG, "%s: NULL in / out, w_max outside [2, %d] or more than %lld problems", who, p->w_max, (long long)p->k_cap);
  const int ctl = in->control & 0x0f;
  if ((in->control & ~0x1f) || (ctl != MPLX_VEL && ctl != MPLX_ACC && ctl != MPLX_JRK))
    return fail(c, MPLX_ERR_ARG, "%s: control must be VEL, ACC or JRK (with or without the yaw bit)", who);
  if (in->yaw_control != MPLX_VEL) return fail(c, MPLX_ERR_ARG, "%s: only yaw_control VEL is built", who);
  *so = control_order(in->control) - 1;
  const int64_t K = in->n_prob;
  if (K > 0 && !in->waypoints) return fail(c, MPLX_ERR_ARG, "%s: NULL waypoints", who);
  if (in->wp_stride < K || (in->dts && in->dt_stride < K) || (in->wp_flags && in->flag_stride < K) ||
      (out->coeff && out->coeff_stride < K) || (out->dts_out && out->dts_out_stride < K) || (out->yaw_coeff && out->yaw_stride < K) ||
      (out->taus && out->taus_stride < K))
    return fail(c, MPLX_ERR_ARG, "%s: a stride is smaller than n_prob", who);
  return MPLX_OK;
}

int solve_launch(mplx_poly *p, const mplx_solve_in *in, const mplx_solve_out *out, int so) {
  mplx_ctx *c = p->c;
  p->n = in->n_prob;
  p->w = in->w_max;
  p->solved = true;
  p->control = in->control;
  p->has_lambda = false;  // a new solve clears the Lambda (include/mplx_scale.h)
  const mplx::TrajArgs t = poly_table_args(p);
  mplx::SolveArgs a{};
  a.n_prob = a.cap = in->n_prob;
  a.w_max = in->w_max;
  a.so = so;
  a.waypoints = in->waypoints; a.wp_stride = in->wp_stride;
  a.n_wp = in->n_wp;
  a.dts = in->dts; a.dt_stride = in->dt_stride;
  a.v = in->v; a.v_arr = in->v_arr;
  a.wp_flags = in->wp_flags; a.flag_stride = in->flag_stride;
  a.tab_S = t.tab_S; a.tab_status = t.tab_status; a.tab_T = t.tab_T; a.tab_tau = t.tab_tau; a.tab_seg = t.tab_seg;
  a.tab_dt = (double *)t.tab_dt; a.tab_wp = (double *)t.tab_wp;
  a.ws = (double *)((char *)p->mem.p + p->o_ws);
  a.status = out->status; a.n_segs = out->n_segs; a.total_time = out->total_time;
  a.coeff = out->coeff; a.coeff_stride = out->coeff_stride;
  a.yaw_coeff = out->yaw_coeff; a.yaw_stride = out->yaw_stride;
  a.dts_out = out->dts_out; a.dts_out_stride = out->dts_out_stride;
  a.taus_out = out->taus; a.taus_stride = out->taus_stride;
  HIP_TRY(c, mplx::launch_solve(c->dim, a, c->stream));
  return MPLX_OK;
}

int check_solved(mplx_poly *p, const char *who, const void *out) {
  if (!out) return fail(p->c, MPLX_ERR_ARG, "%s: NULL out", who);
  if (!p->solved) return fail(p->c, MPLX_ERR_STATE, "%s: nothing has been solved into this poly", who);
  return MPLX_OK;
}

int check_info(mplx_poly *p, const char *who, const mplx_traj_info_out *o) {
  if ((o->effort && o->effort_stride < p->n) || (o->seg_state && o->seg_stride < p->n))
    return fail(p->c, MPLX_ERR_ARG, "%s: effort_stride / seg_stride < n_prob", who);
  return MPLX_OK;
}

int check_times(mplx_poly *p, const char *who, const mplx_traj_times *t, const mplx_traj_sample_out *o, int64_t *count) {
  mplx_ctx *c = p->c;
  if (!t || (t->form != MPLX_TRAJ_COMMAND && t->form != MPLX_TRAJ_WAYPOINT) || t->n_uniform < 0 ||
      (t->n_uniform == 0 && (t->n_times < 1 || t->time_stride < 0 || (t->time_stride != 0 && t->time_stride < t->n_times) ||
                             (p->n > 0 && !t->times))))
    return fail(c, MPLX_ERR_ARG, "%s: bad times (N >= 1, or Q >= 1 values with a stride of 0 or >= Q) or form", who);
  *count = t->n_uniform > 0 ? (int64_t)t->n_uniform + 1 : t->n_times;
  if (o->out && (o->sample_stride < *count || o->row_stride / o->sample_stride < p->n))
    return fail(c, MPLX_ERR_ARG, "%s: sample_stride < samples or row_stride < n_prob * sample_stride", who);
  return MPLX_OK;
}

int check_traverse(mplx_poly *p, const char *who, int32_t lanes) {
  mplx_ctx *c = p->c;
  if (lanes != 0 && lanes != 4 && lanes != 16 && lanes != 64) return fail(c, MPLX_ERR_ARG, "%s: lanes must be 0, 4, 16 or 64", who);
  if (p->has_lambda) return fail(c, MPLX_ERR_STATE, "%s: the poly holds a Lambda; time scaling does not move the path: mplx_poly_clear_lambda first", who);
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "%s: set the map first", who);
  if (c->n_cells > 0x7fffffffLL) return fail(c, MPLX_ERR_STATE, "%s: the map has more cells than getIndex (int32) can number", who);
  if (!(c->prm.v_max > 0)) return fail(c, MPLX_ERR_STATE, "%s: v_max must be > 0 (env_map.h:231)", who);
  return MPLX_OK;
}

int info_launch(mplx_poly *p, const mplx_traj_info_out *o) {
  mplx::TrajArgs a = poly_table_args(p);
  a.status = o->status; a.n_segs = o->n_segs; a.total_time = o->total_time;
  a.effort = o->effort; a.effort_stride = o->effort_stride;
  a.seg_state = o->seg_state; a.seg_stride = o->seg_stride;
  HIP_TRY(p->c, mplx::launch_poly_info(p->c->dim, a, p->c->stream));
  if (p->has_lambda && o->total_time) return poly_lambda_total(p, o->total_time);  // the scaled total (include/mplx_scale.h)
  return MPLX_OK;
}

int sample_launch(mplx_poly *p, const mplx_traj_times *t, const mplx_traj_sample_out *o, int64_t count) {
  mplx_ctx *c = p->c;
  if (o->status) {
    mplx_traj_info_out io{};
    io.status = o->status;
    if (int rc = info_launch(p, &io)) return rc;
  }
  if (!o->out) return MPLX_OK;
  mplx::TrajArgs a = poly_table_args(p);
  a.n_uniform = t->n_uniform; a.times = t->times; a.time_stride = t->n_uniform > 0 ? 0 : t->time_stride; a.count = count;
  a.out = o->out; a.row_stride = o->row_stride; a.sample_stride = o->sample_stride;
  HIP_TRY(c, mplx::launch_traj_sample(c->dim, t->form, a, c->stream));
  return MPLX_OK;
}

// lanes == 0: the durations are on the device, so no bound on the samples is known here; 16 lanes per trajectory, the
// middle one of traj_api.cpp's rule
int traverse_launch(mplx_poly *p, int32_t lanes, const mplx_traj_traverse_out *o) {
  mplx::TrajArgs a = poly_table_args(p);
  a.status = o->status; a.cost = o->cost; a.n_samples = o->n_samples; a.n_cells = o->n_cells; a.stop_sample = o->stop_sample;
  HIP_TRY(p->c, mplx::launch_traj_traverse(p->c->dim, lanes ? lanes : 16, a, p->c->stream));
  return MPLX_OK;
}

// the S_k of the last solve or load, for the host twins: they decide which rows exist
StageRows::Row counts_row(mplx_poly *p, StageRows *s) { return s->landed_from((char *)p->mem.p + p->o_S, (size_t)p->n * 4); }

}  // namespace

extern "C" {

int mplx_poly_create(mplx_ctx *c, int64_t k_cap, int32_t w_max, mplx_poly **out) {
  if (!c) return MPLX_ERR_ARG;
  if (!out || k_cap < 1 || w_max < 2) return fail(c, MPLX_ERR_ARG, "mplx_poly_create: NULL out, k_cap < 1 or w_max < 2");
  *out = nullptr;
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  mplx_poly *p = new mplx_poly;
  p->c = c;
  p->k_cap = k_cap;
  p->w_max = w_max;
  const size_t K = (size_t)k_cap, W = (size_t)w_max, D = (size_t)c->dim;
  StageLayout l;  // (only the carving)
  p->o_S = l.add(K * 4); p->o_st = l.add(K); p->o_T = l.add(K * 8); p->o_tau = l.add(W * K * 8);
  p->o_seg = l.add((W - 1) * (6 * D + 2) * K * 8); p->o_dt = l.add((W - 1) * K * 8); p->o_wp = l.add((4 * D + 2) * W * K * 8);
  p->o_ws = l.add(W * (9 + 3 * D) * K * 8);
  if (int rc = ensure(c, p->mem, l.total)) {
    delete p;
    return rc;
  }
  *out = p;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

void mplx_poly_destroy(mplx_poly *p) {
  if (!p) return;
  (void)hipSetDevice(p->c->device);
  (void)hipStreamSynchronize(p->c->stream);
  release(p->mem);
  release(p->aux);
  release(p->lam);
  release(p->conf);
  delete p;
}

int mplx_solve_device(mplx_poly *p, const mplx_solve_in *d_in, const mplx_solve_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  int so = 0;
  if (int rc = check_in(p, "mplx_solve_device", d_in, d_out, &so)) return rc;
  if (d_in->n_prob == 0) return MPLX_OK;
  if (int rc = bind_device(p->c)) return rc;
  return solve_launch(p, d_in, d_out, so);
}

int mplx_solve(mplx_poly *p, const mplx_solve_in *h_in, const mplx_solve_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  int so = 0;
  if (int rc = check_in(p, "mplx_solve", h_in, h_out, &so)) return rc;
  if (h_in->n_prob == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t n = (size_t)h_in->n_prob, W = (size_t)h_in->w_max, D = (size_t)c->dim, F = 4 * D + 2, N = 2 * ((size_t)so + 1);
  const size_t cr = (W - 1) * N * D;  // coefficient rows
  StageRows s;
  const auto i_wp = s.in_rows(h_in->waypoints, (size_t)h_in->wp_stride * 8, n * 8, F * W), i_nwp = s.in(h_in->n_wp, n * 4),
             i_dts = s.in_rows(h_in->dts, (size_t)h_in->dt_stride * 8, n * 8, W - 1), i_v = s.in(h_in->v_arr, n * 8),
             i_fl = s.in_rows(h_in->wp_flags, (size_t)h_in->flag_stride, n, W);
  const auto o_st = s.landed(n), o_S = s.scratch(n * 4), o_T = s.landed(n * 8), o_c = s.landed(h_out->coeff, cr * n * 8),
             o_d = s.landed(h_out->dts_out, (W - 1) * n * 8), o_y = s.landed(h_out->yaw_coeff, 2 * (W - 1) * n * 8),
             o_t = s.landed(h_out->taus, W * n * 8), t_S = s.landed_from((char *)p->mem.p + p->o_S, n * 4);  // (S_k: 0 for a failed problem)
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_solve_in in = *h_in;
  in.waypoints = s.dev<double>(i_wp); in.wp_stride = (int64_t)n;
  in.n_wp = s.dev<int32_t>(i_nwp);
  in.dts = s.dev<double>(i_dts); in.dt_stride = (int64_t)n;
  in.v_arr = s.dev<double>(i_v);
  in.wp_flags = s.dev<uint8_t>(i_fl); in.flag_stride = (int64_t)n;
  mplx_solve_out o{};
  o.status = s.dev<uint8_t>(o_st); o.n_segs = s.dev<int32_t>(o_S); o.total_time = s.dev<double>(o_T);
  o.coeff = s.dev<double>(o_c); o.dts_out = s.dev<double>(o_d); o.yaw_coeff = s.dev<double>(o_y); o.taus = s.dev<double>(o_t);
  o.coeff_stride = o.dts_out_stride = o.yaw_stride = o.taus_stride = (int64_t)n;
  if (int rc = solve_launch(p, &in, &o, so)) return rc;
  if (int rc = stage_fetch(c, &s)) return rc;
  const uint8_t *st = s.host<uint8_t>(o_st);
  const int32_t *S = s.host<int32_t>(t_S);
  const double *T = s.host<double>(o_T), *cf = s.host<double>(o_c), *dt = s.host<double>(o_d), *yw = s.host<double>(o_y), *ta = s.host<double>(o_t);
  // a failed problem: its status only; rows past S_k keep the caller's bytes
  for (size_t k = 0; k < n; k++) {
    if (h_out->status) h_out->status[k] = st[k];
    const size_t Sk = (size_t)S[k];
    if (Sk == 0) continue;
    if (h_out->n_segs) h_out->n_segs[k] = S[k];
    if (h_out->total_time) h_out->total_time[k] = T[k];
    for (size_t r = 0; r < Sk * N * D && h_out->coeff; r++) h_out->coeff[(int64_t)r * h_out->coeff_stride + (int64_t)k] = cf[r * n + k];
    for (size_t r = 0; r < Sk && h_out->dts_out; r++) h_out->dts_out[(int64_t)r * h_out->dts_out_stride + (int64_t)k] = dt[r * n + k];
    for (size_t r = 0; r < 2 * Sk && h_out->yaw_coeff; r++) h_out->yaw_coeff[(int64_t)r * h_out->yaw_stride + (int64_t)k] = yw[r * n + k];
    for (size_t r = 0; r <= Sk && h_out->taus; r++) h_out->taus[(int64_t)r * h_out->taus_stride + (int64_t)k] = ta[r * n + k];
  }
  return MPLX_OK;
}

int mplx_poly_info_device(mplx_poly *p, const mplx_traj_info_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_solved(p, "mplx_poly_info_device", d_out)) return rc;
  if (int rc = check_info(p, "mplx_poly_info_device", d_out)) return rc;
  if (int rc = bind_device(p->c)) return rc;
  return info_launch(p, d_out);
}

int mplx_poly_info(mplx_poly *p, const mplx_traj_info_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_solved(p, "mplx_poly_info", h_out)) return rc;
  if (int rc = check_info(p, "mplx_poly_info", h_out)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)p->n, F = 4 * (size_t)c->dim + 2, W = (size_t)p->w;
  StageRows s;
  const auto o_st = s.landed(n), o_T = s.landed(n * 8), o_e = s.landed(h_out->effort, 5 * n * 8), o_seg = s.landed(h_out->seg_state, F * W * n * 8),
             t_S = counts_row(p, &s);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_traj_info_out o{};
  o.status = s.dev<uint8_t>(o_st);
  o.total_time = s.dev<double>(o_T);
  o.effort = s.dev<double>(o_e);
  o.effort_stride = (int64_t)n;
  o.seg_state = s.dev<double>(o_seg);
  o.seg_stride = (int64_t)n;
  if (int rc = info_launch(p, &o)) return rc;
  if (int rc = stage_fetch(c, &s)) return rc;
  const uint8_t *st = s.host<uint8_t>(o_st);
  const int32_t *S = s.host<int32_t>(t_S);
  const double *T = s.host<double>(o_T), *e = s.host<double>(o_e), *seg = s.host<double>(o_seg);
  for (size_t k = 0; k < n; k++) {
    if (h_out->status) h_out->status[k] = st[k];
    if (S[k] == 0) continue;
    if (h_out->n_segs) h_out->n_segs[k] = S[k];
    if (h_out->total_time) h_out->total_time[k] = T[k];
    for (size_t r = 0; r < 5 && h_out->effort; r++) h_out->effort[(int64_t)r * h_out->effort_stride + (int64_t)k] = e[r * n + k];
    if (h_out->seg_state)
      for (size_t f = 0; f < F; f++)
        for (size_t w = 0; w <= (size_t)S[k]; w++) h_out->seg_state[(int64_t)(f * W + w) * h_out->seg_stride + (int64_t)k] = seg[(f * W + w) * n + k];
  }
  return MPLX_OK;
}

int mplx_poly_sample_device(mplx_poly *p, const mplx_traj_times *d_times, const mplx_traj_sample_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  int64_t count = 0;
  if (int rc = check_solved(p, "mplx_poly_sample_device", d_out)) return rc;
  if (int rc = check_times(p, "mplx_poly_sample_device", d_times, d_out, &count)) return rc;
  if (int rc = bind_device(p->c)) return rc;
  return sample_launch(p, d_times, d_out, count);
}

int mplx_poly_sample(mplx_poly *p, const mplx_traj_times *h_times, const mplx_traj_sample_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  int64_t count = 0;
  if (int rc = check_solved(p, "mplx_poly_sample", h_out)) return rc;
  if (int rc = check_times(p, "mplx_poly_sample", h_times, h_out, &count)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)p->n, cnt = (size_t)count, D = (size_t)c->dim;
  const size_t rows = h_times->form == MPLX_TRAJ_COMMAND ? 4 * D + 3 : 4 * D + 1;
  const bool own_times = h_times->n_uniform == 0;
  const size_t n_cols = own_times ? (h_times->time_stride ? n : 1) : 0;
  const size_t src_stride = (size_t)(h_times->time_stride ? h_times->time_stride : (int64_t)cnt) * 8;
  StageRows s;
  const auto i_t = s.in_rows(own_times ? h_times->times : nullptr, src_stride, cnt * 8, n_cols), o_st = s.out_or_scratch(h_out->status, n),
             o_out = s.landed(h_out->out, rows * n * cnt * 8), t_S = counts_row(p, &s);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_traj_times t = *h_times;
  if (own_times) {
    t.times = s.dev<double>(i_t);
    t.time_stride = h_times->time_stride ? (int64_t)cnt : 0;
  }
  mplx_traj_sample_out o{};
  o.out = s.dev<double>(o_out);
  o.sample_stride = (int64_t)cnt;
  o.row_stride = (int64_t)(n * cnt);
  o.status = s.dev<uint8_t>(o_st);
  if (int rc = sample_launch(p, &t, &o, count)) return rc;
  if (int rc = stage_fetch(c, &s)) return rc;
  const int32_t *S = s.host<int32_t>(t_S);
  const double *buf = s.host<double>(o_out);
  if (h_out->out)
    for (size_t r = 0; r < rows; r++)
      for (size_t k = 0; k < n; k++) {
        if (S[k] == 0) continue;  // a failed problem keeps the caller's bytes
        std::copy(buf + (r * n + k) * cnt, buf + (r * n + k + 1) * cnt,
                  h_out->out + (int64_t)r * h_out->row_stride + (int64_t)k * h_out->sample_stride);
      }
  return MPLX_OK;
}

int mplx_poly_traverse_device(mplx_poly *p, int32_t lanes, const mplx_traj_traverse_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_solved(p, "mplx_poly_traverse_device", d_out)) return rc;
  if (int rc = check_traverse(p, "mplx_poly_traverse_device", lanes)) return rc;
  if (int rc = bind_device(p->c)) return rc;
  return traverse_launch(p, lanes, d_out);
}

int mplx_poly_traverse(mplx_poly *p, int32_t lanes, const mplx_traj_traverse_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_solved(p, "mplx_poly_traverse", h_out)) return rc;
  if (int rc = check_traverse(p, "mplx_poly_traverse", lanes)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)p->n;
  StageRows s;
  const auto o_st = s.out(h_out->status, n), o_cost = s.out(h_out->cost, n * 8), o_ns = s.out(h_out->n_samples, n * 4),
             o_nc = s.out(h_out->n_cells, n * 4), o_stop = s.out(h_out->stop_sample, n * 4);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_traj_traverse_out o{};
  o.status = s.dev<uint8_t>(o_st); o.cost = s.dev<double>(o_cost); o.n_samples = s.dev<int32_t>(o_ns);
  o.n_cells = s.dev<int32_t>(o_nc); o.stop_sample = s.dev<int32_t>(o_stop);
  if (int rc = traverse_launch(p, lanes, &o)) return rc;
  return stage_fetch(c, &s);
}

}  // extern "C"
