// reserve_api.cpp -- C ABI of include/mplx_reserve.h: the reservation table (filled by the init and position launches of
// conflict_kernel.hip, on one chunk of n_steps instants) and the check of successor lists against it
// (reserve_kernel.hip).  The table and the queries are the mplx_reserve's own memory; launches go to the context's
// stream and the host-pointer twins stage their [K] rows through the context's arena.
#include "mplx_poly.h"
#include "../../include/mplx_reserve.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace mplx_detail;

struct mplx_reserve {
  mplx_ctx *c = nullptr;
  DevBuf mem;      // the per-trajectory rows, then pos [D][n_steps][B] and act [n_steps][B]
  DevBuf queries;  // t0 [Q], radius [Q], ignore [Q]
  bool filled = false;
  int32_t Q = 0;
  int64_t B = 0;
  int32_t n_steps = 0;
  double step = 0;
  size_t o_incl = 0, o_st = 0, o_r = 0, o_g = 0, o_pos = 0, o_act = 0;
  size_t q_t0 = 0, q_r = 0, q_ign = 0;
};

namespace {

constexpr int64_t kMaxEntries = 0x7ffffffeLL;  // as the node table's relax

int check_in(mplx_ctx *c, const char *who, const mplx_conflict_in *in) {
  if (!in) return fail(c, MPLX_ERR_ARG, "%s: NULL in", who);
  if (!(in->step > 0) || !std::isfinite(in->step)) return fail(c, MPLX_ERR_ARG, "%s: step must be > 0 and finite", who);
  if (in->n_steps < 1) return fail(c, MPLX_ERR_ARG, "%s: n_steps must be >= 1", who);
  if (in->mode != MPLX_CONFLICT_PARK && in->mode != MPLX_CONFLICT_GONE)
    return fail(c, MPLX_ERR_ARG, "%s: mode must be MPLX_CONFLICT_PARK or MPLX_CONFLICT_GONE", who);
  return MPLX_OK;
}

int check_size(mplx_ctx *c, const char *who, int64_t K, const mplx_conflict_in *in) {
  const int64_t per = 8 * (int64_t)c->dim + 1;
  if (K > 0 && (int64_t)in->n_steps > (int64_t)MPLX_RESERVE_MAX_BYTES / per / K)
    return fail(c, MPLX_ERR_ARG, "%s: %lld trajectories x %d instants exceed MPLX_RESERVE_MAX_BYTES", who, (long long)K, (int)in->n_steps);
  return MPLX_OK;
}

// the init and position launches on the table `t`, into the reserve's own memory
int fill(mplx_reserve *r, const mplx::TrajArgs &t, const mplx_conflict_in *in) {
  mplx_ctx *c = r->c;
  const size_t K = (size_t)t.n_traj, D = (size_t)c->dim, n = (size_t)in->n_steps;
  r->filled = false;
  StageLayout l;  // (only the carving)
  const size_t o_incl = l.add(K), o_st = l.add(K), o_r = l.add(K * 8), o_t0 = l.add(K * 8), o_g = l.add(K * 4), o_rk = l.add(K * 4),
               o_af = l.add(K * 8), o_am = l.add(K * 8), o_pos = l.add(D * n * K * 8), o_act = l.add(n * K);
  if (int rc = ensure(c, r->mem, std::max<size_t>(l.total, 256))) return rc;
  char *b = (char *)r->mem.p;
  mplx::ConflictArgs a{};
  a.traj = t;
  a.K = t.n_traj;
  a.step = in->step; a.n_steps = in->n_steps; a.gone = in->mode == MPLX_CONFLICT_GONE;
  a.t0 = in->t0; a.radius = in->radius; a.radius_all = in->radius_all; a.group = in->group; a.rank = nullptr;
  a.m_incl = (uint8_t *)(b + o_incl); a.m_status = (uint8_t *)(b + o_st); a.m_r = (double *)(b + o_r); a.m_t0 = (double *)(b + o_t0);
  a.m_group = (int32_t *)(b + o_g); a.m_rank = (int32_t *)(b + o_rk);
  a.acc_first = (unsigned long long *)(b + o_af); a.acc_min = (unsigned long long *)(b + o_am);
  a.pos = (double *)(b + o_pos); a.act = (uint8_t *)(b + o_act);
  a.chunk = in->n_steps; a.c0 = 0; a.cn = in->n_steps;
  HIP_TRY(c, mplx::launch_conflict_positions(c->dim, a, c->stream));
  r->o_incl = o_incl; r->o_st = o_st; r->o_r = o_r; r->o_g = o_g; r->o_pos = o_pos; r->o_act = o_act;
  r->B = t.n_traj; r->n_steps = in->n_steps; r->step = in->step;
  r->filled = true;
  return MPLX_OK;
}

// the [K] rows of a host mplx_conflict_in in the arena; after the commit, the device form of `h_in`
struct Rows { StageRows::Row t0, radius, group; };
Rows rows_of(size_t K, const mplx_conflict_in *in, StageRows *s) {
  const auto t0 = s->in(in->t0, K * 8), radius = s->in(in->radius, K * 8);
  return {t0, radius, s->in(in->group, K * 4)};
}
mplx_conflict_in staged_in(const StageRows &s, const Rows &r, const mplx_conflict_in *h_in) {
  mplx_conflict_in in = *h_in;
  in.rank = nullptr;
  in.t0 = s.dev<double>(r.t0); in.radius = s.dev<double>(r.radius); in.group = s.dev<int32_t>(r.group);
  return in;
}

int check_poly(mplx_reserve *r, mplx_poly *p, const char *who, const mplx_conflict_in *in) {
  mplx_ctx *c = r->c;
  if (!p) return fail(c, MPLX_ERR_ARG, "%s: NULL poly", who);
  if (p->c != c) return fail(c, MPLX_ERR_ARG, "%s: the poly belongs to another context", who);
  if (int rc = check_in(c, who, in)) return rc;
  if (!p->solved) return fail(c, MPLX_ERR_STATE, "%s: nothing has been solved or loaded into this poly", who);
  return check_size(c, who, p->n, in);
}

int check_traj(mplx_reserve *r, mplx_ctx *ctx, const char *who, const mplx_traj_set *s, const mplx_conflict_in *in) {
  mplx_ctx *c = r->c;
  if (ctx != c) return fail(c, MPLX_ERR_ARG, "%s: the reservation table belongs to another context", who);
  if (!s) return fail(c, MPLX_ERR_ARG, "%s: NULL set", who);
  if (int rc = check_in(c, who, in)) return rc;
  if (int rc = traj_check_set(c, who, s, in)) return rc;
  return check_size(c, who, s->n_traj, in);
}

}  // namespace

int mplx_detail::reserve_fill_args(mplx_reserve *r, const char *who, mplx_ctx **c, mplx::ReserveArgs *a) {
  *c = r->c;
  if (!r->filled) return fail(r->c, MPLX_ERR_STATE, "%s: the reservation table has not been filled", who);
  const char *b = (const char *)r->mem.p, *qb = (const char *)r->queries.p;
  a->pos = (const double *)(b + r->o_pos); a->act = (const uint8_t *)(b + r->o_act); a->incl = (const uint8_t *)(b + r->o_incl);
  a->r = (const double *)(b + r->o_r); a->group = (const int32_t *)(b + r->o_g);
  a->B = r->B; a->n_steps = r->n_steps; a->step = r->step;
  a->Q = r->Q;
  if (r->Q < 1) return MPLX_OK;
  a->q_t0 = (const double *)(qb + r->q_t0); a->q_r = (const double *)(qb + r->q_r); a->q_ignore = (const int32_t *)(qb + r->q_ign);
  return MPLX_OK;
}

int mplx_detail::reserve_table_args(mplx_reserve *r, const char *who, mplx_ctx **c, mplx::ReserveArgs *a) {
  if (int rc = reserve_fill_args(r, who, c, a)) return rc;
  if (r->Q < 1) return fail(r->c, MPLX_ERR_STATE, "%s: mplx_reserve_set_queries has not been called", who);
  mplx_ctx *x = r->c;
  a->U = (const double *)x->U.p; a->nU = x->nU; a->udim = x->udim;
  a->dt = x->prm.dt;
  const double scan = std::ceil(x->prm.dt / r->step) + 3.0;  // as mplx_reserve_check_device
  a->n_scan = scan < 2147483647.0 ? (int32_t)scan : 0x7fffffff;
  return MPLX_OK;
}

extern "C" {

int mplx_reserve_create(mplx_ctx *c, mplx_reserve **out) {
  if (!c) return MPLX_ERR_ARG;
  if (!out) return fail(c, MPLX_ERR_ARG, "mplx_reserve_create: NULL out");
  *out = nullptr;
  MPLX_GUARD_BEGIN
  mplx_reserve *r = new mplx_reserve;
  r->c = c;
  *out = r;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

void mplx_reserve_destroy(mplx_reserve *r) {
  if (!r) return;
  (void)hipSetDevice(r->c->device);
  (void)hipStreamSynchronize(r->c->stream);
  release(r->mem);
  release(r->queries);
  delete r;
}

int mplx_reserve_fill_poly_device(mplx_reserve *r, mplx_poly *p, const mplx_conflict_in *d_in) {
  if (!r) return MPLX_ERR_ARG;
  if (int rc = check_poly(r, p, "mplx_reserve_fill_poly_device", d_in)) return rc;
  if (int rc = bind_device(r->c)) return rc;
  return fill(r, poly_table_args(p), d_in);
}

int mplx_reserve_fill_poly(mplx_reserve *r, mplx_poly *p, const mplx_conflict_in *h_in) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = r->c;
  if (int rc = check_poly(r, p, "mplx_reserve_fill_poly", h_in)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t K = (size_t)p->n;
  StageRows s;
  const Rows rows = rows_of(K, h_in, &s);
  if (int rc = stage_commit(c, &s)) return rc;
  const mplx_conflict_in in = staged_in(s, rows, h_in);
  if (int rc = fill(r, poly_table_args(p), &in)) return rc;
  return stage_fetch(c, &s);
}

int mplx_reserve_fill_traj_device(mplx_reserve *r, mplx_ctx *ctx, const mplx_traj_set *d_set, const mplx_conflict_in *d_in) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = r->c;
  if (int rc = check_traj(r, ctx, "mplx_reserve_fill_traj_device", d_set, d_in)) return rc;
  if (int rc = bind_device(c)) return rc;
  mplx::TrajArgs t{};
  if (d_set->n_traj > 0)
    if (int rc = traj_build_table(c, d_set, &t)) return rc;
  return fill(r, t, d_in);
}

int mplx_reserve_fill_traj(mplx_reserve *r, mplx_ctx *ctx, const mplx_traj_set *h_set, const mplx_conflict_in *h_in) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = r->c;
  if (int rc = check_traj(r, ctx, "mplx_reserve_fill_traj", h_set, h_in)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t K = (size_t)h_set->n_traj;
  mplx::TrajArgs t{};
  if (K == 0) return fill(r, t, h_in);
  StageRows s;
  const TrajSetRows set = traj_set_rows(c, h_set, &s);
  const Rows rows = rows_of(K, h_in, &s);
  if (int rc = stage_commit(c, &s)) return rc;
  const mplx_traj_set d = traj_set_view(h_set, s, set);
  const mplx_conflict_in in = staged_in(s, rows, h_in);
  if (int rc = traj_build_table(c, &d, &t)) return rc;
  if (int rc = fill(r, t, &in)) return rc;
  return stage_fetch(c, &s);
}

int mplx_reserve_shape(mplx_reserve *r, int64_t *n_traj, int32_t *n_steps, double *step) {
  if (!r) return MPLX_ERR_ARG;
  if (!r->filled) return fail(r->c, MPLX_ERR_STATE, "mplx_reserve_shape: the table has not been filled");
  if (n_traj) *n_traj = r->B;
  if (n_steps) *n_steps = r->n_steps;
  if (step) *step = r->step;
  return MPLX_OK;
}

int mplx_reserve_positions(mplx_reserve *r, double *h_pos, uint8_t *h_active, uint8_t *h_included, double *h_radius, int32_t *h_group,
                           uint8_t *h_status) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = r->c;
  if (!r->filled) return fail(c, MPLX_ERR_STATE, "mplx_reserve_positions: the table has not been filled");
  if (int rc = bind_device(c)) return rc;
  if (r->B == 0) return MPLX_OK;
  const size_t B = (size_t)r->B, D = (size_t)c->dim, n = (size_t)r->n_steps;
  const char *b = (const char *)r->mem.p;
  // the device keeps [D][n_steps][B]; the caller gets [n_steps][D][B]
  for (size_t d = 0; d < D && h_pos; d++)
    HIP_TRY(c, stage_out_rows(c, h_pos + d * B, D * B * 8, b + r->o_pos + d * n * B * 8, B * 8, n));
  HIP_TRY(c, stage_out(c, h_active, b + r->o_act, n * B));
  HIP_TRY(c, stage_out(c, h_included, b + r->o_incl, B));
  HIP_TRY(c, stage_out(c, h_radius, b + r->o_r, B * 8));
  HIP_TRY(c, stage_out(c, h_group, b + r->o_g, B * 4));
  HIP_TRY(c, stage_out(c, h_status, b + r->o_st, B));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

int mplx_reserve_set_queries(mplx_reserve *r, int32_t Q, const double *h_t0, const double *h_radius, const int32_t *h_ignore) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = r->c;
  const char *who = "mplx_reserve_set_queries";
  if (Q < 1 || Q > 65536 || !h_t0 || !h_radius) return fail(c, MPLX_ERR_ARG, "%s: need 1 <= Q <= 65536, h_t0 and h_radius", who);
  for (int32_t q = 0; q < Q; q++) {
    if (!std::isfinite(h_t0[q]) || !(h_t0[q] >= 0)) return fail(c, MPLX_ERR_ARG, "%s: t0[%d] must be finite and >= 0", who, (int)q);
    if (!std::isfinite(h_radius[q]) || !(h_radius[q] >= 0)) return fail(c, MPLX_ERR_ARG, "%s: radius[%d] must be finite and >= 0", who, (int)q);
  }
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  StageLayout l;  // (only the carving)
  const size_t o_t0 = l.add((size_t)Q * 8), o_r = l.add((size_t)Q * 8), o_ign = l.add((size_t)Q * 4);
  r->Q = 0;
  if (int rc = ensure(c, r->queries, l.total)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // a check in flight reads the old values
  std::vector<int32_t> ign((size_t)Q, -1);
  if (h_ignore) std::copy(h_ignore, h_ignore + Q, ign.begin());
  char *b = (char *)r->queries.p;
  HIP_TRY(c, hipMemcpy(b + o_t0, h_t0, (size_t)Q * 8, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(b + o_r, h_radius, (size_t)Q * 8, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(b + o_ign, ign.data(), (size_t)Q * 4, hipMemcpyHostToDevice));
  r->q_t0 = o_t0; r->q_r = o_r; r->q_ign = o_ign;
  r->Q = Q;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

int mplx_reserve_check_device(mplx_reserve *r, mplx_table *tab, const mplx_succ_lists *L, int64_t n_nodes, const int32_t *d_parent_id,
                              const double *d_parent_state, int64_t parent_stride, int64_t *d_hit, int64_t *d_n_blocked) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = r->c;
  const char *who = "mplx_reserve_check_device";
  if (!L || n_nodes < 0 || !d_parent_id || !d_parent_state) return fail(c, MPLX_ERR_ARG, "%s: NULL argument or n_nodes < 0", who);
  if (!L->count || !L->action || !L->cost) return fail(c, MPLX_ERR_ARG, "%s: the lists need count, action and cost", who);
  const int64_t S = list_stride(c, L);
  if (S < 1 || n_nodes > kMaxEntries / S) return fail(c, MPLX_ERR_ARG, "%s: node_stride < 1 or more than 2^31 - 2 list entries", who);
  if (parent_stride < n_nodes) return fail(c, MPLX_ERR_ARG, "%s: parent_stride < n_nodes", who);
  const int32_t *d_query = nullptr;
  int32_t tab_Q = 1;
  int64_t tab_cap = 0;
  if (tab) {
    mplx_ctx *tc = nullptr;
    const int rc = table_reserve_args(tab, who, &tc, &d_query, &tab_Q, &tab_cap);  // (sets tc whatever it answers)
    if (tc != c) return fail(c, MPLX_ERR_ARG, "%s: the table belongs to another context", who);
    if (rc) return rc;
  }
  if (!r->filled) return fail(c, MPLX_ERR_STATE, "%s: the table has not been filled", who);
  if (r->Q < 1) return fail(c, MPLX_ERR_STATE, "%s: mplx_reserve_set_queries has not been called", who);
  if (tab_Q != r->Q) return fail(c, MPLX_ERR_ARG, "%s: %d queries were set, the table has %d", who, (int)r->Q, (int)tab_Q);
  if (!c->has_params) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_params has not been called", who);
  if (!c->has_U) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_controls has not been called", who);
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // yaw pinning: the lists must be final
  if (n_nodes == 0) return MPLX_OK;
  const char *b = (const char *)r->mem.p, *qb = (const char *)r->queries.p;
  mplx::ReserveArgs a{};
  a.pos = (const double *)(b + r->o_pos); a.act = (const uint8_t *)(b + r->o_act); a.incl = (const uint8_t *)(b + r->o_incl);
  a.r = (const double *)(b + r->o_r); a.group = (const int32_t *)(b + r->o_g);
  a.B = r->B; a.n_steps = r->n_steps; a.step = r->step;
  a.q_t0 = (const double *)(qb + r->q_t0); a.q_r = (const double *)(qb + r->q_r); a.q_ignore = (const int32_t *)(qb + r->q_ign);
  a.Q = r->Q;
  a.node_query = tab_Q > 1 ? d_query : nullptr;
  a.node_cap = tab_cap;
  a.count = L->count; a.action = L->action; a.cost = L->cost;
  a.n_rows = n_nodes; a.S = S;
  a.parent_id = d_parent_id; a.parent_state = d_parent_state; a.parent_stride = parent_stride;
  a.U = (const double *)c->U.p; a.nU = c->nU; a.udim = c->udim;
  a.dt = c->prm.dt;
  const double scan = std::ceil(c->prm.dt / r->step) + 3.0;
  a.n_scan = scan < 2147483647.0 ? (int32_t)scan : 0x7fffffff;  // (the scan also ends at n_steps)
  // lanes over a row's entries: the smallest power of two >= S, at least 8, 64 at the most; the other lanes of the
  // wave split the reservations (mplx_ctx::Tuning::reserve_lanes forces 2^k lanes over the entries, for measurements)
  int sp = 3;
  while ((1 << sp) < 64 && (1 << sp) < S) sp++;
  for (int k = 0; k <= 6; k++)
    if (c->tune.reserve_lanes == (1 << k)) sp = k;
  a.sp_log2 = sp;
  a.hit = (long long *)d_hit;
  a.n_blocked = (unsigned long long *)d_n_blocked;
  HIP_TRY(c, mplx::launch_reserve_check(c->dim, c->prm.control, a, c->stream));
  return MPLX_OK;
}

int mplx_reserve_park_device(mplx_reserve *r, mplx_open *o, const mplx_table_frontier *f, int64_t n_max, int64_t *d_hit,
                             int64_t *d_n_vetoed) {
  if (!r) return MPLX_ERR_ARG;
  mplx_ctx *c = r->c;
  const char *who = "mplx_reserve_park_device";
  if (!o || n_max < 0) return fail(c, MPLX_ERR_ARG, "%s: NULL open set or n_max < 0", who);
  if (!f || !f->id || !f->state || !f->count || f->capacity < 0 || f->state_stride < f->capacity)
    return fail(c, MPLX_ERR_ARG, "%s: the frontier needs id, state and count, and state_stride >= capacity >= 0", who);
  mplx_ctx *oc = nullptr;
  mplx_table *tab = nullptr;
  mplx::OpenArgs oa{};
  const int orc = open_park_args(o, who, &oc, &tab, &oa);  // (sets oc whatever it answers)
  if (oc != c) return fail(c, MPLX_ERR_ARG, "%s: the open set belongs to another context", who);
  if (orc) return orc;
  if (!r->filled) return fail(c, MPLX_ERR_STATE, "%s: the table has not been filled", who);
  if (r->Q < 1) return fail(c, MPLX_ERR_STATE, "%s: mplx_reserve_set_queries has not been called", who);
  if (oa.n_queries != r->Q) return fail(c, MPLX_ERR_ARG, "%s: %d queries were set, the table has %d", who, (int)r->Q, (int)oa.n_queries);
  const int64_t rows = std::min(n_max, f->capacity);
  if (rows == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  const char *b = (const char *)r->mem.p, *qb = (const char *)r->queries.p;
  mplx::ParkArgs a{};
  a.res.pos = (const double *)(b + r->o_pos); a.res.act = (const uint8_t *)(b + r->o_act); a.res.incl = (const uint8_t *)(b + r->o_incl);
  a.res.r = (const double *)(b + r->o_r); a.res.group = (const int32_t *)(b + r->o_g);
  a.res.B = r->B; a.res.n_steps = r->n_steps; a.res.step = r->step;
  a.res.q_t0 = (const double *)(qb + r->q_t0); a.res.q_r = (const double *)(qb + r->q_r); a.res.q_ignore = (const int32_t *)(qb + r->q_ign);
  a.res.Q = r->Q;
  a.res.node_query = oa.n_queries > 1 ? oa.t_query : nullptr;
  a.res.node_cap = oa.cap;
  a.t_n_nodes = &oa.t_ctl->n_nodes;
  a.flags = oa.flags;
  a.f_id = f->id; a.f_state = f->state; a.f_stride = f->state_stride; a.f_cap = f->capacity; a.f_count = f->count;
  a.n_max = n_max;
  a.n_scan = 4;  // the guess is floor(x) - 1 with x within a few ulps of the first instant's index
  a.hit = (long long *)d_hit;
  a.n_vetoed = (unsigned long long *)d_n_vetoed;
  HIP_TRY(c, mplx::launch_reserve_park(c->dim, a, rows, c->stream));
  return MPLX_OK;
}

}  // extern "C"
