// reserve_poly_api.cpp -- C ABI of the check of include/mplx_reserve_poly.h: the problems of a poly against a reservation
// table (reserve_poly_kernel.hip).  The table is the mplx_reserve's own memory, the segment table the poly's; the launch
// goes to the context's stream and the host-pointer twin stages its [K] rows through the context's arena like every other
// twin and is synchronous.  The timed shortcut of the same header stands next to the shortcut it extends,
// in limits_api.cpp.
#include "mplx_poly.h"
#include "../../include/mplx_reserve_poly.h"

using namespace mplx_detail;

int mplx_detail::reserve_check_poly_launch(const mplx::ReserveArgs &t, mplx_poly *p, const double *d_t_start, const double *d_radius,
                                           double radius_all, const int32_t *d_ignore, int64_t *d_hit, uint8_t *d_status,
                                           int64_t *d_n_hit) {
  mplx_ctx *c = p->c;
  mplx::ReservePolyArgs a{};
  a.res = t;
  a.traj = poly_table_args(p);
  a.K = p->n;
  a.t_start = d_t_start; a.radius = d_radius; a.radius_all = radius_all; a.ignore = d_ignore;
  a.hit = (long long *)d_hit; a.status = d_status; a.n_hit = (unsigned long long *)d_n_hit;
  HIP_TRY(c, mplx::launch_reserve_check_poly(c->dim, a, c->stream));
  return MPLX_OK;
}

namespace {

int check(mplx_reserve *r, mplx_poly *p, const char *who, const mplx_reserve_poly_in *in, const mplx_reserve_poly_out *out,
          mplx_ctx **ctx, mplx::ReserveArgs *t) {
  mplx_ctx *c = nullptr;
  const int rc = reserve_fill_args(r, who, &c, t);  // (sets c whatever it answers)
  *ctx = c;
  if (!p) return fail(c, MPLX_ERR_ARG, "%s: NULL poly", who);
  if (p->c != c) return fail(c, MPLX_ERR_ARG, "%s: the poly belongs to another context", who);
  if (!in || !out) return fail(c, MPLX_ERR_ARG, "%s: NULL in / out", who);
  if (rc) return rc;
  if (!p->solved) return fail(c, MPLX_ERR_STATE, "%s: nothing has been solved or loaded into this poly", who);
  if (p->n > 0 && !in->t_start) return fail(c, MPLX_ERR_ARG, "%s: NULL t_start", who);
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_reserve_check_poly_device(mplx_reserve *r, mplx_poly *p, const mplx_reserve_poly_in *d_in, const mplx_reserve_poly_out *d_out) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = nullptr;
  mplx::ReserveArgs t{};
  if (int rc = check(r, p, "mplx_reserve_check_poly_device", d_in, d_out, &c, &t)) return rc;
  if (p->n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  return reserve_check_poly_launch(t, p, d_in->t_start, d_in->radius, d_in->radius_all, d_in->ignore_group, d_out->hit, d_out->status,
                                   d_out->n_hit);
}

int mplx_reserve_check_poly(mplx_reserve *r, mplx_poly *p, const mplx_reserve_poly_in *h_in, const mplx_reserve_poly_out *h_out) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = nullptr;
  mplx::ReserveArgs t{};
  if (int rc = check(r, p, "mplx_reserve_check_poly", h_in, h_out, &c, &t)) return rc;
  if (p->n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t K = (size_t)p->n;
  StageRows s;
  const auto i_t = s.in(h_in->t_start, K * 8), i_r = s.in(h_in->radius, K * 8), i_g = s.in(h_in->ignore_group, K * 4);
  const auto o_h = s.out(h_out->hit, K * 8), o_s = s.out(h_out->status, K), o_n = s.inout(h_out->n_hit, 8);
  if (int rc = stage_commit(c, &s)) return rc;
  if (int rc = reserve_check_poly_launch(t, p, s.dev<double>(i_t), s.dev<double>(i_r), h_in->radius_all, s.dev<int32_t>(i_g),
                                         s.dev<int64_t>(o_h), s.dev<uint8_t>(o_s), s.dev<int64_t>(o_n)))
    return rc;
  return stage_fetch(c, &s);
}

}  // extern "C"
