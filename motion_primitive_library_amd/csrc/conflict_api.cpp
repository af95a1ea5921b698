// conflict_api.cpp -- C ABI of include/mplx_conflict.h: conflicts between the trajectories of one set on a common clock
// (conflict_kernel.hip).  The set is a poly's segment table or the one the chain launch of traj_api.cpp leaves in the
// context; the scratch (per-trajectory rows, accumulators, the positions of one chunk of instants) is the poly's or the
// context's own.  The host-pointer twins stage their [K] rows through the context's arena.
#include "mplx_poly.h"
#include "../../include/mplx_conflict.h"

#include <algorithm>
#include <cmath>

using namespace mplx_detail;

namespace {

int check_in(mplx_ctx *c, const char *who, int64_t K, const mplx_conflict_in *in, const mplx_conflict_out *out) {
  if (!in || !out) return fail(c, MPLX_ERR_ARG, "%s: NULL in / out", who);
  if (!(in->step > 0) || !std::isfinite(in->step)) return fail(c, MPLX_ERR_ARG, "%s: step must be > 0 and finite", who);
  if (in->n_steps < 1) return fail(c, MPLX_ERR_ARG, "%s: n_steps must be >= 1", who);
  if (in->mode != MPLX_CONFLICT_PARK && in->mode != MPLX_CONFLICT_GONE)
    return fail(c, MPLX_ERR_ARG, "%s: mode must be MPLX_CONFLICT_PARK or MPLX_CONFLICT_GONE", who);
  if (in->chunk_steps < 0) return fail(c, MPLX_ERR_ARG, "%s: chunk_steps < 0", who);
  if (out->pair_first && out->pair_stride < K) return fail(c, MPLX_ERR_ARG, "%s: pair_stride < K", who);
  return MPLX_OK;
}

// instants per pass: the caller's, or as many as keep the position table under MPLX_CONFLICT_SCRATCH_BYTES (one at least)
int32_t chunk_of(int dim, int64_t K, const mplx_conflict_in *in) {
  if (in->chunk_steps > 0) return std::min(in->chunk_steps, in->n_steps);
  const int64_t per = K * (8 * (int64_t)dim + 1);
  const int64_t fit = (int64_t)MPLX_CONFLICT_SCRATCH_BYTES / std::max<int64_t>(per, 1);
  return (int32_t)std::min<int64_t>(std::max<int64_t>(fit, 1), in->n_steps);
}

// init, the chunks, final -- on the table `t`, with scratch `ws`
int run(mplx_ctx *c, DevBuf &ws, const mplx::TrajArgs &t, const mplx_conflict_in *in, const mplx_conflict_out *o) {
  const size_t K = (size_t)t.n_traj, D = (size_t)c->dim;
  const int32_t chunk = chunk_of(c->dim, t.n_traj, in);
  StageLayout l;  // (only the carving)
  const size_t o_incl = l.add(K), o_st = l.add(K), o_r = l.add(K * 8), o_t0 = l.add(K * 8), o_g = l.add(K * 4), o_rk = l.add(K * 4),
               o_af = l.add(K * 8), o_am = l.add(K * 8), o_pos = l.add(D * (size_t)chunk * K * 8), o_act = l.add((size_t)chunk * K);
  if (int rc = ensure(c, ws, l.total)) return rc;
  char *b = (char *)ws.p;
  mplx::ConflictArgs a{};
  a.traj = t;
  a.K = t.n_traj;
  a.step = in->step; a.n_steps = in->n_steps; a.gone = in->mode == MPLX_CONFLICT_GONE;
  a.t0 = in->t0; a.radius = in->radius; a.radius_all = in->radius_all; a.group = in->group; a.rank = in->rank;
  a.m_incl = (uint8_t *)(b + o_incl); a.m_status = (uint8_t *)(b + o_st); a.m_r = (double *)(b + o_r); a.m_t0 = (double *)(b + o_t0);
  a.m_group = (int32_t *)(b + o_g); a.m_rank = (int32_t *)(b + o_rk);
  a.acc_first = (unsigned long long *)(b + o_af); a.acc_min = (unsigned long long *)(b + o_am);
  a.pos = (double *)(b + o_pos); a.act = (uint8_t *)(b + o_act);
  a.chunk = chunk;
  a.first_step = o->first_step; a.first_partner = o->first_partner; a.min_d2 = o->min_d2; a.status = o->status;
  a.pair_first = o->pair_first; a.pair_stride = o->pair_stride;
  HIP_TRY(c, mplx::launch_conflict_init(a, c->stream));
  for (int32_t c0 = 0; c0 < in->n_steps; c0 += chunk) {
    a.c0 = c0;
    a.cn = std::min(chunk, in->n_steps - c0);
    HIP_TRY(c, mplx::launch_conflict_chunk(c->dim, a, c->stream));
  }
  HIP_TRY(c, mplx::launch_conflict_final(a, c->stream));
  return MPLX_OK;
}

// the [K] rows of a host call in the arena; after the commit, the device forms of `h_in` and `h_out`
struct Rows { StageRows::Row t0, radius, group, rank, first, partner, d2, status, pairs; };
Rows rows_of(size_t K, const mplx_conflict_in *in, const mplx_conflict_out *o, StageRows *s) {
  Rows r;
  r.t0 = s->in(in->t0, K * 8); r.radius = s->in(in->radius, K * 8);
  r.group = s->in(in->group, K * 4); r.rank = s->in(in->rank, K * 4);
  r.first = s->out(o->first_step, K * 4); r.partner = s->out(o->first_partner, K * 4);
  r.d2 = s->out(o->min_d2, K * 8); r.status = s->out(o->status, K);
  r.pairs = s->out_rows(o->pair_first, (size_t)o->pair_stride * 4, K * 4, K);
  return r;
}
void staged(const StageRows &s, const Rows &r, size_t K, const mplx_conflict_in *h_in, mplx_conflict_in *in, mplx_conflict_out *o) {
  *in = *h_in;
  in->t0 = s.dev<double>(r.t0); in->radius = s.dev<double>(r.radius); in->group = s.dev<int32_t>(r.group); in->rank = s.dev<int32_t>(r.rank);
  *o = mplx_conflict_out{};
  o->first_step = s.dev<int32_t>(r.first); o->first_partner = s.dev<int32_t>(r.partner); o->min_d2 = s.dev<double>(r.d2);
  o->status = s.dev<uint8_t>(r.status); o->pair_first = s.dev<int32_t>(r.pairs);
  o->pair_stride = (int64_t)K;
}

int check_poly(mplx_poly *p, const char *who, const mplx_conflict_in *in, const mplx_conflict_out *out) {
  if (int rc = check_in(p->c, who, p->solved ? p->n : 0, in, out)) return rc;
  if (!p->solved) return fail(p->c, MPLX_ERR_STATE, "%s: nothing has been solved or loaded into this poly", who);
  return MPLX_OK;
}

int check_traj(mplx_ctx *c, const char *who, const mplx_traj_set *s, const mplx_conflict_in *in, const mplx_conflict_out *out) {
  if (!s) return fail(c, MPLX_ERR_ARG, "%s: NULL set", who);
  if (int rc = check_in(c, who, s->n_traj, in, out)) return rc;
  return traj_check_set(c, who, s, out);
}

}  // namespace

extern "C" {

int mplx_poly_conflicts_device(mplx_poly *p, const mplx_conflict_in *d_in, const mplx_conflict_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_poly(p, "mplx_poly_conflicts_device", d_in, d_out)) return rc;
  if (p->n == 0) return MPLX_OK;
  if (int rc = bind_device(p->c)) return rc;
  return run(p->c, p->conf, poly_table_args(p), d_in, d_out);
}

int mplx_poly_conflicts(mplx_poly *p, const mplx_conflict_in *h_in, const mplx_conflict_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_poly(p, "mplx_poly_conflicts", h_in, h_out)) return rc;
  if (p->n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t K = (size_t)p->n;
  StageRows s;
  const Rows r = rows_of(K, h_in, h_out, &s);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_conflict_in in;
  mplx_conflict_out o;
  staged(s, r, K, h_in, &in, &o);
  if (int rc = run(c, p->conf, poly_table_args(p), &in, &o)) return rc;
  return stage_fetch(c, &s);
}

int mplx_traj_conflicts_device(mplx_ctx *c, const mplx_traj_set *d_set, const mplx_conflict_in *d_in, const mplx_conflict_out *d_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_traj(c, "mplx_traj_conflicts_device", d_set, d_in, d_out)) return rc;
  if (d_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  mplx::TrajArgs t;
  if (int rc = traj_build_table(c, d_set, &t)) return rc;
  return run(c, c->conflict_ws, t, d_in, d_out);
}

int mplx_traj_conflicts(mplx_ctx *c, const mplx_traj_set *h_set, const mplx_conflict_in *h_in, const mplx_conflict_out *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_traj(c, "mplx_traj_conflicts", h_set, h_in, h_out)) return rc;
  if (h_set->n_traj == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t K = (size_t)h_set->n_traj;
  StageRows s;
  const TrajSetRows set = traj_set_rows(c, h_set, &s);
  const Rows r = rows_of(K, h_in, h_out, &s);
  if (int rc = stage_commit(c, &s)) return rc;
  const mplx_traj_set d = traj_set_view(h_set, s, set);
  mplx_conflict_in in;
  mplx_conflict_out o;
  staged(s, r, K, h_in, &in, &o);
  mplx::TrajArgs t;
  if (int rc = traj_build_table(c, &d, &t)) return rc;
  if (int rc = run(c, c->conflict_ws, t, &in, &o)) return rc;
  return stage_fetch(c, &s);
}

}  // extern "C"
