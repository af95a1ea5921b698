// scale_api.cpp -- C ABI of include/mplx_scale.h: the Lambda of every problem of an mplx_poly (scale_kernel.hip).  The
// poly's Lambda table is compact (stride n), so the host-pointer twins run the device form without outputs and read the
// table back; only their inputs, and the rows of mplx_poly_tau, stage through the context's arena.
#include "mplx_poly.h"
#include "../../include/mplx_scale.h"

#include <algorithm>

using namespace mplx_detail;

namespace {

int check_poly(mplx_poly *p, const char *who, const void *in, const void *out, int mode) {
  mplx_ctx *c = p->c;
  if (!in || !out) return fail(c, MPLX_ERR_ARG, "%s: NULL in / out", who);
  if (mode != MPLX_SCALE_REFERENCE && mode != MPLX_SCALE_ROBUST)
    return fail(c, MPLX_ERR_ARG, "%s: mode must be MPLX_SCALE_REFERENCE or MPLX_SCALE_ROBUST", who);
  if (!p->solved) return fail(c, MPLX_ERR_STATE, "%s: nothing has been solved or loaded into this poly", who);
  return MPLX_OK;
}

int check_lambda_out(mplx_poly *p, const char *who, const mplx_lambda_out *o) {
  if ((o->Ts && o->ts_stride < p->n) || (o->segs && o->seg_stride < p->n))
    return fail(p->c, MPLX_ERR_ARG, "%s: ts_stride / seg_stride < n_prob", who);
  return MPLX_OK;
}

// the Lambda table and the scratch rows, on first use
int ensure_lambda(mplx_poly *p) {
  if (p->lam.p) return MPLX_OK;
  const size_t K = (size_t)p->k_cap, W = (size_t)p->w_max;
  StageLayout l;  // (only the carving)
  p->l_n = l.add(K * 4); p->l_st = l.add(K); p->l_seg = l.add(8 * 8 * K * 8); p->l_Ts = l.add(W * K * 8); p->l_total = l.add(K * 8);
  p->l_pts = l.add(9 * 3 * K * 8); p->l_npts = l.add(K * 4); p->l_scaled = l.add(K); p->l_down = l.add((W - 1) * 3 * K * 8);
  p->l_res = l.add(3 * K * 8);
  return ensure(p->c, p->lam, l.total);
}

mplx::ScaleArgs base_args(mplx_poly *p, int mode) {
  const mplx::TrajArgs t = poly_table_args(p);
  char *b = (char *)p->lam.p;
  mplx::ScaleArgs a{};
  a.n_prob = p->n;
  a.w_max = p->w;
  a.robust = mode == MPLX_SCALE_ROBUST;
  a.tab_S = t.tab_S; a.tab_T = t.tab_T; a.tab_tau = t.tab_tau; a.tab_seg = t.tab_seg; a.tab_dt = t.tab_dt;
  a.lam_n = (int32_t *)(b + p->l_n); a.lam_status = (uint8_t *)(b + p->l_st); a.lam_seg = (double *)(b + p->l_seg);
  a.lam_Ts = (double *)(b + p->l_Ts); a.lam_total = (double *)(b + p->l_total);
  a.w_pts = (double *)(b + p->l_pts); a.w_npts = (int32_t *)(b + p->l_npts); a.w_scaled = (uint8_t *)(b + p->l_scaled);
  a.down_seg = (double *)(b + p->l_down); a.w_res = (double *)(b + p->l_res);
  return a;
}

void set_out(mplx::ScaleArgs &a, const mplx_lambda_out *o) {
  a.status = o->status; a.n_lseg = o->n_lseg; a.total = o->total;
  a.Ts = o->Ts; a.ts_stride = o->ts_stride; a.segs = o->segs; a.seg_stride = o->seg_stride;
}

// every build call: the table exists; the poly holds no Lambda until the launches are queued (end_build)
int begin_build(mplx_poly *p) {
  if (int rc = bind_device(p->c)) return rc;
  if (int rc = ensure_lambda(p)) return rc;
  p->has_lambda = false;
  return MPLX_OK;
}

void end_build(mplx_poly *p, int mode) {
  p->has_lambda = true;
  p->lam_mode = mode;
}

int set_lambda_launch(mplx_poly *p, const mplx_lambda_in *in, const mplx_lambda_out *o) {
  if (int rc = begin_build(p)) return rc;
  mplx::ScaleArgs a = base_args(p, in->mode);
  a.pts = in->pts; a.pts_stride = in->stride; a.n_pts = in->n_pts;
  set_out(a, o);
  HIP_TRY(p->c, mplx::launch_lambda_build(a, p->c->stream));
  end_build(p, in->mode);
  return MPLX_OK;
}

int scale_launch(mplx_poly *p, const mplx_scale_in *in, const mplx_lambda_out *o) {
  if (int rc = begin_build(p)) return rc;
  mplx::ScaleArgs a = base_args(p, in->mode);
  a.ri = in->ri; a.rf = in->rf; a.ri_arr = in->ri_arr; a.rf_arr = in->rf_arr;
  set_out(a, o);
  HIP_TRY(p->c, mplx::launch_lambda_scale(a, p->c->stream));
  end_build(p, in->mode);
  return MPLX_OK;
}

int scale_down_launch(mplx_poly *p, const mplx_scale_down_in *in, const mplx_scale_down_out *o) {
  if (int rc = begin_build(p)) return rc;
  mplx::ScaleArgs a = base_args(p, in->mode);
  a.mv = in->mv; a.ma = in->ma; a.ri = in->ri; a.rf = in->rf;
  a.scaled = o->scaled; a.max_l = o->max_l; a.t_lo = o->t_lo; a.t_hi = o->t_hi;
  set_out(a, &o->lambda);
  HIP_TRY(p->c, mplx::launch_lambda_scale_down(p->c->dim, a, p->c->stream));
  end_build(p, in->mode);
  return MPLX_OK;
}

// The host side of a build: the poly's own compact rows (none of them in the arena; the table exists from here on),
// declared before the commit and scattered into the caller's strides after the launch.  A problem with a solve or load status, or one scale_down left
// alone (`down`), keeps the caller's bytes; one with a Lambda status its status.
struct BuildRows { StageRows::Row S, nl, st, total, Ts, segs, sc, res; };
int build_rows(mplx_poly *p, const mplx_lambda_out *h, bool down, StageRows *s, BuildRows *out) {
  if (int rc = ensure_lambda(p)) return rc;
  const size_t n = (size_t)p->n, W = (size_t)p->w;
  const char *b = (const char *)p->lam.p;
  BuildRows &r = *out;
  r.S = s->landed_from((const char *)p->mem.p + p->o_S, n * 4);
  r.nl = s->landed_from(b + p->l_n, n * 4); r.st = s->landed_from(b + p->l_st, n); r.total = s->landed_from(b + p->l_total, n * 8);
  r.Ts = s->landed_from(b + p->l_Ts, h->Ts ? W * n * 8 : 0); r.segs = s->landed_from(b + p->l_seg, h->segs ? 64 * n * 8 : 0);
  r.sc = s->landed_from(b + p->l_scaled, down ? n : 0); r.res = s->landed_from(b + p->l_res, down ? 3 * n * 8 : 0);
  return MPLX_OK;
}
int read_back(mplx_poly *p, StageRows *s, const BuildRows &r, const mplx_lambda_out *h, const mplx_scale_down_out *down) {
  if (int rc = stage_fetch(p->c, s)) return rc;
  const size_t n = (size_t)p->n;
  const int32_t *S = s->host<int32_t>(r.S), *nl = s->host<int32_t>(r.nl);
  const uint8_t *st = s->host<uint8_t>(r.st), *sc = s->host<uint8_t>(r.sc);
  const double *total = s->host<double>(r.total), *Ts = s->host<double>(r.Ts), *segs = s->host<double>(r.segs), *res = s->host<double>(r.res);
  if (down && std::none_of(sc, sc + n, [](uint8_t x) { return x != 0; }))
    p->has_lambda = false;  // nothing was scaled: the poly is a plain one again (sample, traverse)
  for (size_t k = 0; k < n; k++) {
    if (S[k] == 0) continue;
    if (down) {
      if (down->scaled) down->scaled[k] = sc[k];
      if (!sc[k]) continue;
      if (down->max_l) down->max_l[k] = res[k];
      if (down->t_lo) down->t_lo[k] = res[n + k];
      if (down->t_hi) down->t_hi[k] = res[2 * n + k];
    }
    if (h->status) h->status[k] = st[k];
    if (st[k]) continue;
    if (h->n_lseg) h->n_lseg[k] = nl[k];
    if (h->total) h->total[k] = total[k];
    for (size_t s = 0; s <= (size_t)S[k] && h->Ts; s++) h->Ts[(int64_t)s * h->ts_stride + (int64_t)k] = Ts[s * n + k];
    for (size_t r = 0; r < (size_t)nl[k] * 8 && h->segs; r++) h->segs[(int64_t)r * h->seg_stride + (int64_t)k] = segs[r * n + k];
  }
  return MPLX_OK;
}

int check_tau(mplx_poly *p, const char *who, const mplx_traj_times *t, const mplx_tau_out *o, int64_t *count) {
  mplx_ctx *c = p->c;
  if (!o) return fail(c, MPLX_ERR_ARG, "%s: NULL out", who);
  if (!p->solved) return fail(c, MPLX_ERR_STATE, "%s: nothing has been solved or loaded into this poly", who);
  if (!p->has_lambda) return fail(c, MPLX_ERR_STATE, "%s: the poly holds no Lambda", who);
  if (!t || t->n_uniform < 0 ||
      (t->n_uniform == 0 && (t->n_times < 1 || t->time_stride < 0 || (t->time_stride != 0 && t->time_stride < t->n_times) ||
                             (p->n > 0 && !t->times))))
    return fail(c, MPLX_ERR_ARG, "%s: bad times (N >= 1, or Q >= 1 values with a stride of 0 or >= Q)", who);
  *count = t->n_uniform > 0 ? (int64_t)t->n_uniform + 1 : t->n_times;
  if ((o->tau || o->lambda || o->lambda_dot || o->found) && o->stride < *count)
    return fail(c, MPLX_ERR_ARG, "%s: stride < samples", who);
  return MPLX_OK;
}

int tau_launch(mplx_poly *p, const mplx_traj_times *t, const mplx_tau_out *o, int64_t count) {
  mplx::ScaleArgs a = base_args(p, p->lam_mode);
  a.n_uniform = t->n_uniform; a.times = t->times; a.time_stride = t->n_uniform > 0 ? 0 : t->time_stride; a.count = count;
  a.tau = o->tau; a.lam = o->lambda; a.lam_dot = o->lambda_dot; a.found = o->found; a.out_stride = o->stride;
  HIP_TRY(p->c, mplx::launch_lambda_tau(a, p->c->stream));
  return MPLX_OK;
}

}  // namespace

namespace mplx_detail {

int poly_lambda_total(mplx_poly *p, double *d_total_time) {
  mplx::ScaleArgs a = base_args(p, p->lam_mode);
  a.total_time = d_total_time;
  HIP_TRY(p->c, mplx::launch_lambda_total(a, p->c->stream));
  return MPLX_OK;
}

}  // namespace mplx_detail

extern "C" {

int mplx_poly_set_lambda_device(mplx_poly *p, const mplx_lambda_in *d_in, const mplx_lambda_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_poly(p, "mplx_poly_set_lambda_device", d_in, d_out, d_in ? d_in->mode : 0)) return rc;
  if (int rc = check_lambda_out(p, "mplx_poly_set_lambda_device", d_out)) return rc;
  if (p->n > 0 && (!d_in->pts || d_in->stride < p->n)) return fail(p->c, MPLX_ERR_ARG, "mplx_poly_set_lambda_device: NULL pts or stride < n_prob");
  return set_lambda_launch(p, d_in, d_out);
}

int mplx_poly_set_lambda(mplx_poly *p, const mplx_lambda_in *h_in, const mplx_lambda_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_poly(p, "mplx_poly_set_lambda", h_in, h_out, h_in ? h_in->mode : 0)) return rc;
  if (int rc = check_lambda_out(p, "mplx_poly_set_lambda", h_out)) return rc;
  if (p->n > 0 && (!h_in->pts || h_in->stride < p->n)) return fail(c, MPLX_ERR_ARG, "mplx_poly_set_lambda: NULL pts or stride < n_prob");
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t n = (size_t)p->n;
  StageRows s;
  const auto i_p = s.in_rows(h_in->pts, (size_t)h_in->stride * 8, n * 8, 27), i_n = s.in(h_in->n_pts, n * 4);
  BuildRows rb;
  if (int rc = build_rows(p, h_out, false, &s, &rb)) return rc;
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_lambda_in in = *h_in;
  in.pts = s.dev<double>(i_p); in.stride = (int64_t)n;
  in.n_pts = s.dev<int32_t>(i_n);
  const mplx_lambda_out none{};
  if (int rc = set_lambda_launch(p, &in, &none)) return rc;
  return read_back(p, &s, rb, h_out, nullptr);
}

int mplx_poly_scale_device(mplx_poly *p, const mplx_scale_in *d_in, const mplx_lambda_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_poly(p, "mplx_poly_scale_device", d_in, d_out, d_in ? d_in->mode : 0)) return rc;
  if (int rc = check_lambda_out(p, "mplx_poly_scale_device", d_out)) return rc;
  return scale_launch(p, d_in, d_out);
}

int mplx_poly_scale(mplx_poly *p, const mplx_scale_in *h_in, const mplx_lambda_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_poly(p, "mplx_poly_scale", h_in, h_out, h_in ? h_in->mode : 0)) return rc;
  if (int rc = check_lambda_out(p, "mplx_poly_scale", h_out)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)p->n;
  StageRows s;
  const auto i_ri = s.in(h_in->ri_arr, n * 8), i_rf = s.in(h_in->rf_arr, n * 8);
  BuildRows rb;
  if (int rc = build_rows(p, h_out, false, &s, &rb)) return rc;
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_scale_in in = *h_in;
  in.ri_arr = s.dev<double>(i_ri);
  in.rf_arr = s.dev<double>(i_rf);
  const mplx_lambda_out none{};
  if (int rc = scale_launch(p, &in, &none)) return rc;
  return read_back(p, &s, rb, h_out, nullptr);
}

int mplx_poly_scale_down_device(mplx_poly *p, const mplx_scale_down_in *in, const mplx_scale_down_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_poly(p, "mplx_poly_scale_down_device", in, d_out, in ? in->mode : 0)) return rc;
  if (int rc = check_lambda_out(p, "mplx_poly_scale_down_device", &d_out->lambda)) return rc;
  return scale_down_launch(p, in, d_out);
}

int mplx_poly_scale_down(mplx_poly *p, const mplx_scale_down_in *in, const mplx_scale_down_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_poly(p, "mplx_poly_scale_down", in, h_out, in ? in->mode : 0)) return rc;
  if (int rc = check_lambda_out(p, "mplx_poly_scale_down", &h_out->lambda)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  StageRows s;  // (no arena row: the build reads no host array)
  BuildRows rb;
  if (int rc = build_rows(p, &h_out->lambda, true, &s, &rb)) return rc;
  if (int rc = stage_commit(c, &s)) return rc;
  const mplx_scale_down_out none{};
  if (int rc = scale_down_launch(p, in, &none)) return rc;
  return read_back(p, &s, rb, &h_out->lambda, h_out);
}

int mplx_poly_tau_device(mplx_poly *p, const mplx_traj_times *d_times, const mplx_tau_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  int64_t count = 0;
  if (int rc = check_tau(p, "mplx_poly_tau_device", d_times, d_out, &count)) return rc;
  if (int rc = bind_device(p->c)) return rc;
  return tau_launch(p, d_times, d_out, count);
}

int mplx_poly_tau(mplx_poly *p, const mplx_traj_times *h_times, const mplx_tau_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  int64_t count = 0;
  if (int rc = check_tau(p, "mplx_poly_tau", h_times, h_out, &count)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)p->n, cnt = (size_t)count;
  const bool own_times = h_times->n_uniform == 0;
  const size_t n_cols = own_times ? (h_times->time_stride ? n : 1) : 0;
  const size_t src_stride = (size_t)(h_times->time_stride ? h_times->time_stride : (int64_t)cnt) * 8;
  StageRows s;
  const auto i_t = s.in_rows(own_times ? h_times->times : nullptr, src_stride, cnt * 8, n_cols), o_tau = s.landed(n * cnt * 8),
             o_l = s.landed(n * cnt * 8), o_d = s.landed(n * cnt * 8), o_f = s.landed(n * cnt),
             t_S = s.landed_from((char *)p->mem.p + p->o_S, n * 4);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_traj_times t = *h_times;
  if (own_times) {
    t.times = s.dev<double>(i_t);
    t.time_stride = h_times->time_stride ? (int64_t)cnt : 0;
  }
  mplx_tau_out o{};
  o.tau = s.dev<double>(o_tau); o.lambda = s.dev<double>(o_l); o.lambda_dot = s.dev<double>(o_d);
  o.found = s.dev<uint8_t>(o_f); o.stride = (int64_t)cnt;
  if (int rc = tau_launch(p, &t, &o, count)) return rc;
  if (int rc = stage_fetch(c, &s)) return rc;
  const int32_t *S = s.host<int32_t>(t_S);
  const double *tau = s.host<double>(o_tau), *lam = s.host<double>(o_l), *dot = s.host<double>(o_d);
  const uint8_t *fd = s.host<uint8_t>(o_f);
  for (size_t k = 0; k < n; k++) {
    if (S[k] == 0) continue;  // a failed problem keeps the caller's bytes
    const int64_t at = (int64_t)k * h_out->stride;
    if (h_out->tau) std::copy(tau + k * cnt, tau + (k + 1) * cnt, h_out->tau + at);
    if (h_out->lambda) std::copy(lam + k * cnt, lam + (k + 1) * cnt, h_out->lambda + at);
    if (h_out->lambda_dot) std::copy(dot + k * cnt, dot + (k + 1) * cnt, h_out->lambda_dot + at);
    if (h_out->found) std::copy(fd + k * cnt, fd + (k + 1) * cnt, h_out->found + at);
  }
  return MPLX_OK;
}

int mplx_poly_clear_lambda(mplx_poly *p) {
  if (!p) return MPLX_ERR_ARG;
  p->has_lambda = false;  // the table's rows are dead: the next build rewrites every problem's
  return MPLX_OK;
}

}  // extern "C"
