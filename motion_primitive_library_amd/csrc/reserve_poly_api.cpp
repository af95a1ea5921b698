// reserve_poly_api.cpp -- C ABI of the check of include/mplx_reserve_poly.h: the problems of a poly against a reservation
// table (reserve_poly_kernel.hip).  The table is the mplx_reserve's own memory, the segment table the poly's; the launch
// goes to the context's stream and the host-pointer twin lays out its [K] rows in the reservation table's own row buffer
// (reserve_host_rows) and is synchronous.  The timed shortcut of the same header stands next to the shortcut it extends,
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
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t K = (size_t)p->n;
  StageLayout l;
  const size_t i_t = l.add(K * 8), i_r = l.add(h_in->radius ? K * 8 : 0), i_g = l.add(h_in->ignore_group ? K * 4 : 0);
  const size_t o_h = l.add(h_out->hit ? K * 8 : 0), o_s = l.add(h_out->status ? K : 0), o_n = l.add(h_out->n_hit ? 8 : 0);
  if (int rc = reserve_host_rows(r, l.total, &l.base)) return rc;
  HIP_TRY(c, stage_in(c, l.base + i_t, h_in->t_start, K * 8));
  if (h_in->radius) HIP_TRY(c, stage_in(c, l.base + i_r, h_in->radius, K * 8));
  if (h_in->ignore_group) HIP_TRY(c, stage_in(c, l.base + i_g, h_in->ignore_group, K * 4));
  if (h_out->n_hit) HIP_TRY(c, stage_in(c, l.base + o_n, h_out->n_hit, 8));
  int64_t *d_hit = h_out->hit ? (int64_t *)(l.base + o_h) : nullptr, *d_n = h_out->n_hit ? (int64_t *)(l.base + o_n) : nullptr;
  uint8_t *d_st = h_out->status ? (uint8_t *)(l.base + o_s) : nullptr;
  if (int rc = reserve_check_poly_launch(t, p, (const double *)(l.base + i_t), h_in->radius ? (const double *)(l.base + i_r) : nullptr,
                                         h_in->radius_all, h_in->ignore_group ? (const int32_t *)(l.base + i_g) : nullptr, d_hit, d_st, d_n))
    return rc;
  HIP_TRY(c, stage_out(c, h_out->hit, d_hit, K * 8));
  HIP_TRY(c, stage_out(c, h_out->status, d_st, K));
  HIP_TRY(c, stage_out(c, h_out->n_hit, d_n, 8));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

}  // extern "C"
