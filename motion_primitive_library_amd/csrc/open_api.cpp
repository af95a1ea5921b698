// open_api.cpp -- C ABI of include/mplx_open.h: the open set of a node table (open_kernel.hip).  The open set's arrays,
// control blocks and scratch are its own; launches go to the stream of the table's context.  No call touches the
// staging arena: push and select take device pointers only.
#include "mplx_ctx.h"
#include "../../include/mplx_anytime.h"
#include "../../include/mplx_best.h"
#include "../../include/mplx_field.h"
#include "../../include/mplx_heur.h"
#include "../../include/mplx_multi.h"
#include "../../include/mplx_prior.h"
#include "../../include/mplx_ray.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace mplx_detail;

static_assert(sizeof(mplx::OpenResult) == sizeof(mplx_open_result), "mplx::OpenResult is mplx_open_result");
static_assert(sizeof(mplx::OpenBound) == sizeof(mplx_open_bound), "mplx::OpenBound is mplx_open_bound");

struct mplx_open {
  mplx_table *tab = nullptr;
  mplx_ctx *c = nullptr;
  int64_t cap = 0;
  int32_t Q = 1;                        // the table's queries: 2 * Q control blocks, Q results in the mirror
  DevBuf f, flags, ctl, mark, tot;
  DevBuf rows;                          // push with the ray trace: per row a flags byte, a count (and a query); grows on demand
  DevBuf goals;                         // mplx_open_set_goals: Q goals (mplx::PostFuse)
  bool has_goals = false;
  double goals_tol = 0.0;               // the largest tol_pos among them: bounds the rays of a push
  mplx::OpenResult *mirror = nullptr;   // pinned, [Q]
  int parity = 0;                       // which control block the next select reduces into
  // include/mplx_prior.h: goals0 = the goals as mplx_open_set_goals gave them (`goals` carries the priors' ends while
  // priors are in force); the table, its scratch and the rows of the view
  DevBuf goals0, pr_n, pr_pos, pr_togo, pr_status, pr_sidx, pr_sterm, pr_costs, pr_trav, pr_grow, pr_ghash;
  bool has_priors = false;
  int64_t pr_cap = 0;                   // steps per query the table is laid out for
  double pr_dt = 0.0;                   // the searching context's dt when the table was built
  // include/mplx_field.h: the goal field in force, the field of every query (device, [Q]) and the largest entry
  mplx_field *fld = nullptr;
  DevBuf fld_q;
  int32_t fld_max = -1;
  bool fld_gone = false;                // the field was destroyed while in force: a push is an error
  double goals_vmin = 0.0;              // the smallest v_max among the goals of mplx_open_set_goals
  // include/mplx_heur.h: the mode of the pushes; control and goal_control of every goal (device, [Q][2]); the smallest w
  int32_t heur_mode = 0;
  DevBuf dyn_ctl;
  double goals_wmin = 0.0;
  // include/mplx_best.h: histograms, states and rank counts of a best-select, allocated by the first one
  DevBuf best;
  // include/mplx_anytime.h: the control blocks, the cut and the pinned mirror of the bound of a re-key ([Q] each), allocated on demand
  DevBuf rk_ctl, rk_cut;
  mplx::OpenBound *rk_mirror = nullptr;
};

namespace {

// the field of `o` is no longer in force (cleared, replaced, dropped by new goals, or the open set goes)
void drop_field(mplx_open *o) {
  if (o->fld) {
    std::vector<mplx_open *> &u = o->fld->users;
    u.erase(std::remove(u.begin(), u.end(), o), u.end());
  }
  o->fld = nullptr;
  o->fld_gone = false;
}

void release_open(mplx_open *o) {
  drop_field(o);
  for (DevBuf *b : {&o->f, &o->flags, &o->ctl, &o->mark, &o->tot, &o->rows, &o->goals, &o->goals0, &o->pr_n, &o->pr_pos, &o->pr_togo,
                    &o->pr_status, &o->pr_sidx, &o->pr_sterm, &o->pr_costs, &o->pr_trav, &o->pr_grow, &o->pr_ghash, &o->fld_q, &o->dyn_ctl, &o->best, &o->rk_ctl, &o->rk_cut})
    release(*b);
  if (o->mirror) (void)hipHostFree(o->mirror);
  if (o->rk_mirror) (void)hipHostFree(o->rk_mirror);
  delete o;
}

// the table's fields (MPLX_ERR_STATE for a table with a status bit) and the open set's own
int open_args(mplx_open *o, const char *who, mplx::OpenArgs *a) {
  mplx_ctx *c = nullptr;
  if (int rc = table_open_args(o->tab, who, &c, a)) return rc;
  a->f = (unsigned long long *)o->f.p;
  a->flags = (uint8_t *)o->flags.p;
  a->ctl = (mplx::OpenCtl *)o->ctl.p + (size_t)o->parity * (size_t)o->Q;
  a->ctl_next = (mplx::OpenCtl *)o->ctl.p + (size_t)(1 - o->parity) * (size_t)o->Q;
  a->mirror = o->mirror;
  a->mark = (uint8_t *)o->mark.p;
  a->tot = (uint32_t *)o->tot.p;
  return MPLX_OK;
}

int check_frontier(mplx_ctx *c, const char *who, const mplx_table_frontier *f) {
  if (!f || !f->id || !f->g || !f->state || !f->count || f->capacity < 0 || f->state_stride < f->capacity)
    return fail(c, MPLX_ERR_ARG, "%s: the frontier needs id, g, state and count, and state_stride >= capacity >= 0", who);
  return MPLX_OK;
}

void set_frontier(mplx::OpenArgs *a, const mplx_table_frontier *f) {
  a->f_id = f->id; a->f_g = f->g; a->f_state = f->state; a->f_stride = f->state_stride; a->f_cap = f->capacity; a->f_count = f->count;
}

// What the heuristic of a push reads, for the push and for the re-key of include/mplx_anytime.h: the goal(s), the priors,
// the goal field (MPLX_ERR_STATE for one that is stale, empty or destroyed) and the mode of mplx_open_set_heur.
int heur_args(mplx_open *o, const char *who, mplx::OpenArgs *ap) {
  mplx_ctx *c = o->c;
  mplx::OpenArgs &a = *ap;
  a.goal = c->goal_fuse;
  a.goals = o->has_goals ? (const mplx::PostFuse *)o->goals.p : nullptr;
  if (o->has_priors && o->has_goals) {
    a.prior_n = (const int32_t *)o->pr_n.p;
    a.prior_pos = (const double *)o->pr_pos.p;
    a.prior_togo = (const double *)o->pr_togo.p;
    a.prior_cap = o->pr_cap;
    a.prior_dt = o->pr_dt;
  }
  if (o->fld_gone) return fail(c, MPLX_ERR_STATE, "%s: the goal field in force was destroyed (mplx_open_clear_field, or set another)", who);
  if (o->fld) {  // include/mplx_field.h
    const mplx_field *fl = o->fld;
    if (fl->epoch != c->blk_epoch) return fail(c, MPLX_ERR_STATE, "%s: the goal field is stale (the map changed since mplx_field_build)", who);
    if (fl->F < 1 || o->fld_max >= fl->F || fl->n_cells != c->n_cells)
      return fail(c, MPLX_ERR_STATE, "%s: the goal field is empty, or was rebuilt with fewer fields than the queries use", who);
    if (!((o->has_goals ? o->goals_vmin : c->goal_fuse.v_max) > 0)) return fail(c, MPLX_ERR_STATE, "%s: a goal field needs v_max > 0", who);
    a.field_dist = (const int32_t *)fl->dist.p;
    a.field_of_query = (const int32_t *)o->fld_q.p;
    a.field_F = fl->F;
    a.field_cells = fl->n_cells;
    for (int i = 0; i < 3; i++) {
      a.field_dim[i] = c->mdim[i];
      a.field_org[i] = c->origin[i];
    }
    a.field_res = c->res;
  }
  if (o->heur_mode == MPLX_HEUR_ROBUST) {  // include/mplx_heur.h
    if (o->has_priors) return fail(c, MPLX_ERR_STATE, "%s: MPLX_HEUR_ROBUST with priors in force (mplx_open_clear_priors, or mplx_open_set_heur(DEFAULT))", who);
    if (!((o->has_goals ? o->goals_wmin : c->goal_fuse.w) > 0)) return fail(c, MPLX_ERR_STATE, "%s: MPLX_HEUR_ROBUST needs w > 0", who);
    a.dyn = MPLX_HEUR_ROBUST;
    a.dyn_control[0] = c->goal_ctl[0];
    a.dyn_control[1] = c->goal_ctl[1];
    a.dyn_controls = o->has_goals ? (const int32_t *)o->dyn_ctl.p : nullptr;
  }
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_open_create(mplx_table *tab, mplx_open **out) {
  if (!tab) return MPLX_ERR_ARG;
  mplx::OpenArgs a{};
  mplx_ctx *c = nullptr;
  int rc = table_open_args(tab, "mplx_open_create", &c, &a);
  if (!out) return fail(c, MPLX_ERR_ARG, "mplx_open_create: NULL out");
  *out = nullptr;
  if (rc) return rc;
  MPLX_GUARD_BEGIN
  if (int rc2 = bind_device(c)) return rc2;
  mplx_open *o = new mplx_open;
  o->tab = tab;
  o->c = c;
  o->cap = a.cap;
  o->Q = a.n_queries;
  const size_t cap = (size_t)a.cap, tiles = (cap + mplx::kTableTile - 1) / mplx::kTableTile;
  if (!rc) rc = ensure(c, o->f, cap * 8);
  if (!rc) rc = ensure(c, o->flags, cap);
  if (!rc) rc = ensure(c, o->ctl, 2 * (size_t)o->Q * sizeof(mplx::OpenCtl));
  if (!rc) rc = ensure(c, o->mark, cap);
  if (!rc) rc = ensure(c, o->tot, tiles * 4);
  if (!rc && hipHostMalloc((void **)&o->mirror, std::max<size_t>(64, (size_t)o->Q * sizeof(mplx::OpenResult)), hipHostMallocCoherent) != hipSuccess)
    rc = fail(c, MPLX_ERR_HIP, "mplx_open_create: hipHostMalloc failed");
  if (!rc && (rc = open_args(o, "mplx_open_create", &a)) == MPLX_OK && mplx::launch_open_clear(a, c->stream) != hipSuccess)
    rc = fail(c, MPLX_ERR_HIP, "mplx_open_create: the clearing launch failed");
  if (rc) {
    (void)hipGetLastError();
    release_open(o);
    return rc;
  }
  *out = o;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

void mplx_open_destroy(mplx_open *o) {
  if (!o) return;
  (void)hipSetDevice(o->c->device);
  (void)hipStreamSynchronize(o->c->stream);
  release_open(o);
}

int mplx_open_clear(mplx_open *o) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  mplx::OpenArgs a{};
  if (int rc = open_args(o, "mplx_open_clear", &a)) return rc;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, mplx::launch_open_clear(a, c->stream));
  return MPLX_OK;
}

int mplx_open_view_of(mplx_open *o, mplx_open_view *v) {
  if (!o) return MPLX_ERR_ARG;
  if (!v) return fail(o->c, MPLX_ERR_ARG, "mplx_open_view_of: NULL view");
  v->f = (const double *)o->f.p;
  v->flags = (const uint8_t *)o->flags.p;
  return MPLX_OK;
}

int mplx_open_push_device(mplx_open *o, const mplx_table_frontier *d_rows, int64_t n_max, double eps, int32_t sight) {
  if (!o) return MPLX_ERR_ARG;
  return open_push(o, "mplx_open_push_device", d_rows, n_max, eps, sight, false);
}

}  // extern "C"

void mplx_detail::open_field_gone(mplx_open *o) {
  o->fld = nullptr;
  o->fld_gone = true;
}

int mplx_detail::open_park_args(mplx_open *o, const char *who, mplx_ctx **c, mplx_table **tab, mplx::OpenArgs *a) {
  *c = o->c;
  *tab = o->tab;
  return open_args(o, who, a);
}

int mplx_detail::open_push(mplx_open *o, const char *who, const mplx_table_frontier *d_rows, int64_t n_max, double eps, int32_t sight,
                           bool closed) {
  mplx_ctx *c = o->c;
  if (n_max < 0 || !(eps >= 0.0) || std::isinf(eps)) return fail(c, MPLX_ERR_ARG, "%s: need n_max >= 0 and a finite eps >= 0", who);
  if (int rc = check_frontier(c, who, d_rows)) return rc;
  if (o->Q > 1 && !o->has_goals) return fail(c, MPLX_ERR_STATE, "%s: no goals (mplx_open_set_goals)", who);
  if (!o->has_goals && !c->has_goal) return fail(c, MPLX_ERR_STATE, "%s: no goal (mplx_set_goal)", who);
  if (sight && !c->has_map) return fail(c, MPLX_ERR_STATE, "%s: the ray trace needs the map (mplx_set_map)", who);
  mplx::OpenArgs a{};
  if (int rc = open_args(o, who, &a)) return rc;
  const int64_t rows = std::min(n_max, d_rows->capacity);
  if (rows == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  set_frontier(&a, d_rows);
  a.n_max = n_max;
  a.eps = eps;
  if (int rc = heur_args(o, who, &a)) return rc;
  if (!sight) {
    HIP_TRY(c, mplx::launch_open_push(c->dim, 0, a, rows, c->stream, closed));
    return MPLX_OK;
  }
  // around the goal passes of ray_kernel.hip: the frontier as `rows` lists of stride 1 with a flags byte each
  const size_t o_cnt = align256((size_t)rows);
  const size_t o_qry = o_cnt + align256((size_t)rows * 4);
  if (int rc = ensure(c, o->rows, o_qry + (a.goals ? (size_t)rows * 4 : 0))) return rc;
  a.row_flags = (uint8_t *)o->rows.p;
  a.row_count = (int32_t *)((char *)o->rows.p + o_cnt);
  a.row_query = a.goals ? (int32_t *)((char *)o->rows.p + o_qry) : nullptr;
  HIP_TRY(c, mplx::launch_open_push(c->dim, 0, a, rows, c->stream, closed));
  mplx_succ_lists L{};
  L.count = a.row_count;
  L.state = d_rows->state;
  L.state_stride = d_rows->state_stride;
  L.node_stride = 1;
  if (a.goals) {
    // rows that do not count keep flags 0 and are no candidates: their row_query is never read
    if (int rc = goal_sight_rows(c, &L, rows, a.row_query, a.goals, o->goals_tol, a.row_flags)) return rc;
  } else if (int rc = mplx_goal_sight_device(c, &L, rows, nullptr, a.row_flags)) {
    return rc;
  }
  HIP_TRY(c, mplx::launch_open_push(c->dim, 1, a, rows, c->stream, closed));
  return MPLX_OK;
}

extern "C" {

int mplx_open_select_device(mplx_open *o, double delta, const mplx_table_frontier *d_out, mplx_open_result *d_result,
                            mplx_open_result *h_result) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_select_device";
  if (o->Q > 1) return fail(c, MPLX_ERR_STATE, "%s: the table has %d queries: mplx_open_select_multi_device", who, (int)o->Q);
  if (!(delta >= 0.0)) return fail(c, MPLX_ERR_ARG, "%s: need delta >= 0", who);
  if (int rc = check_frontier(c, who, d_out)) return rc;
  mplx::OpenArgs a{};
  if (int rc = open_args(o, who, &a)) return rc;
  if (int rc = bind_device(c)) return rc;
  set_frontier(&a, d_out);
  a.delta = delta;
  a.result = (mplx::OpenResult *)d_result;
  a.n_tiles = (std::max<int64_t>(a.n_bound, 1) + mplx::kTableTile - 1) / mplx::kTableTile;
  HIP_TRY(c, mplx::launch_open_select(a, c->stream));
  o->parity = 1 - o->parity;
  if (!h_result) return MPLX_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  table_observe(o->tab);
  if (int rc = table_open_args(o->tab, who, &c, &a)) return rc;  // a status bit: the select did nothing
  const volatile mplx::OpenResult *m = o->mirror;
  h_result->status = m->status; h_result->goal_id = m->goal_id; h_result->count = m->count; h_result->n_open = m->n_open;
  h_result->f_min = m->f_min; h_result->goal_f = m->goal_f; h_result->goal_g = m->goal_g;
  return MPLX_OK;
}

int mplx_open_set_goals(mplx_open *o, const mplx_goal_spec *h_goals, int32_t n) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_set_goals";
  if (!h_goals) return fail(c, MPLX_ERR_ARG, "%s: NULL goals", who);
  if (n != o->Q) return fail(c, MPLX_ERR_ARG, "%s: %d goals for a table of %d queries", who, (int)n, (int)o->Q);
  MPLX_GUARD_BEGIN
  std::vector<mplx::PostFuse> f((size_t)n);
  std::vector<int32_t> ctl(2 * (size_t)n);
  double tol = 0.0, vmin = 0.0, wmin = 0.0;
  for (int32_t q = 0; q < n; q++) {
    if (int rc = goal_fuse_of(c, who, &h_goals[q], &f[(size_t)q])) return rc;
    tol = std::max(tol, f[(size_t)q].tol_pos);
    vmin = (q == 0 || !(f[(size_t)q].v_max >= vmin)) ? f[(size_t)q].v_max : vmin;
    wmin = (q == 0 || !(f[(size_t)q].w >= wmin)) ? f[(size_t)q].w : wmin;
    ctl[2 * (size_t)q] = h_goals[q].control;
    ctl[2 * (size_t)q + 1] = h_goals[q].goal_control;
  }
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t bytes = (size_t)n * sizeof(mplx::PostFuse);
  if (int rc = ensure(c, o->goals, bytes)) return rc;
  if (int rc = ensure(c, o->goals0, bytes)) return rc;
  if (int rc = ensure(c, o->dyn_ctl, ctl.size() * 4)) return rc;
  StageRows s;
  const auto i_g = s.in(f.data(), bytes), i_c = s.in(ctl.data(), ctl.size() * 4);
  if (int rc = stage_commit(c, &s)) return rc;
  HIP_TRY(c, hipMemcpyAsync(o->dyn_ctl.p, s.dev<char>(i_c), ctl.size() * 4, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(o->goals.p, s.dev<char>(i_g), bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(o->goals0.p, s.dev<char>(i_g), bytes, hipMemcpyDeviceToDevice, c->stream));
  if (int rc = stage_fetch(c, &s)) return rc;  // (no output row: the synchronise -- f leaves scope; the arena is free again)
  o->has_priors = false;  // a new goal: the old prior no longer leads to it (include/mplx_prior.h)
  drop_field(o);          // ... and neither does the old field (include/mplx_field.h)
  o->has_goals = true;
  o->goals_tol = tol;
  o->goals_vmin = vmin;
  o->goals_wmin = wmin;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

int mplx_open_select_multi_device(mplx_open *o, double delta, const mplx_table_frontier *d_out, mplx_open_result *d_results,
                                  mplx_open_result *h_results) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_select_multi_device";
  if (!(delta >= 0.0)) return fail(c, MPLX_ERR_ARG, "%s: need delta >= 0", who);
  if (int rc = check_frontier(c, who, d_out)) return rc;
  mplx::OpenArgs a{};
  if (int rc = open_args(o, who, &a)) return rc;
  if (int rc = bind_device(c)) return rc;
  set_frontier(&a, d_out);
  a.delta = delta;
  a.result = (mplx::OpenResult *)d_results;
  a.n_tiles = (std::max<int64_t>(a.n_bound, 1) + mplx::kTableTile - 1) / mplx::kTableTile;
  HIP_TRY(c, mplx::launch_open_select_multi(a, c->stream));
  o->parity = 1 - o->parity;
  if (!h_results) return MPLX_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  table_observe(o->tab);
  if (int rc = table_open_args(o->tab, who, &c, &a)) return rc;  // a status bit: the select did nothing
  const volatile mplx::OpenResult *m = o->mirror;
  for (int32_t q = 0; q < o->Q; q++) {
    mplx_open_result *h = h_results + q;
    h->status = m[q].status; h->goal_id = m[q].goal_id; h->count = m[q].count; h->n_open = m[q].n_open;
    h->f_min = m[q].f_min; h->goal_f = m[q].goal_f; h->goal_g = m[q].goal_g;
  }
  return MPLX_OK;
}

// ---- include/mplx_prior.h ----------------------------------------------------------------------------------------------

int mplx_open_set_priors_device(mplx_open *o, const mplx_prior_source *src, const mplx_traj_set *s, const mplx_prior_info *h_info) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_set_priors_device";
  if (!src || !s) return fail(c, MPLX_ERR_ARG, "%s: NULL source or set", who);
  const int ctl = src->control & 0x0f;
  if ((src->control & ~0x1f) || (ctl != 0x01 && ctl != 0x03 && ctl != 0x07 && ctl != 0x0f))
    return fail(c, MPLX_ERR_ARG, "%s: unknown control flag %d of the source", who, (int)src->control);
  if (!src->U || src->nU < 1 || src->udim < c->dim + ((src->control & 0x10) ? 1 : 0) || !(src->dt > 0.0) || std::isinf(src->dt))
    return fail(c, MPLX_ERR_ARG, "%s: the source needs U, nU >= 1, udim as its control flag asks and a finite dt > 0", who);
  if (s->n_traj != o->Q) return fail(c, MPLX_ERR_ARG, "%s: %lld trajectories for a table of %d queries", who, (long long)s->n_traj, (int)o->Q);
  if (s->horizon < 1 || (s->n_starts != 1 && s->n_starts != s->n_traj) || s->start_stride < s->n_starts || s->action_stride < s->n_traj ||
      !s->starts || !s->actions)
    return fail(c, MPLX_ERR_ARG, "%s: bad trajectory set (horizon >= 1, starts, actions, strides >= counts)", who);
  if (!o->has_goals) return fail(c, MPLX_ERR_STATE, "%s: no goals of the open set's own (mplx_open_set_goals)", who);
  if (o->heur_mode != MPLX_HEUR_DEFAULT) return fail(c, MPLX_ERR_STATE, "%s: MPLX_HEUR_ROBUST is in force (mplx_open_set_heur(DEFAULT) first)", who);
  if (o->fld) return fail(c, MPLX_ERR_STATE, "%s: a goal field is in force (mplx_open_clear_field first)", who);
  if (!c->has_params) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_params has not been called", who);
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "%s: set the map first", who);
  if (c->n_cells > 0x7fffffffLL) return fail(c, MPLX_ERR_STATE, "%s: the map has more cells than getIndex (int32) can number", who);
  if (!(c->prm.v_max > 0)) return fail(c, MPLX_ERR_STATE, "%s: v_max must be > 0 (env_map.h:231)", who);
  if (!(c->prm.dt > 0) || !(c->res > 0)) return fail(c, MPLX_ERR_STATE, "%s: dt and the resolution must be > 0", who);
  {
    mplx::OpenArgs probe{};
    if (int rc = open_args(o, who, &probe)) return rc;  // a table with a status bit
  }
  // the host's bounds: steps t_k < T <= horizon * source dt, samples n + 1 with n = ceil(v_max T / res)
  const double span = (double)s->horizon * src->dt;
  const double kb = std::ceil(span / c->prm.dt) + 2.0, sb = std::ceil(c->prm.v_max * span / c->res) + 3.0;
  const double lim = 268435456.0 / (double)o->Q;  // 2^28 entries
  if (!(kb <= lim) || !(sb <= lim)) return fail(c, MPLX_ERR_ARG, "%s: the prior table would exceed 2^28 entries", who);
  const size_t Q = (size_t)o->Q, K = (size_t)kb, SC = (size_t)sb, D = (size_t)c->dim;
  if (int rc = bind_device(c)) return rc;
  if (int rc = ensure(c, o->pr_n, Q * 4)) return rc;
  if (int rc = ensure(c, o->pr_status, Q)) return rc;
  if (int rc = ensure(c, o->pr_trav, Q * 8)) return rc;
  if (int rc = ensure(c, o->pr_grow, Q * 14 * 8)) return rc;
  if (int rc = ensure(c, o->pr_ghash, Q * 8)) return rc;
  if (int rc = ensure(c, o->pr_pos, Q * K * D * 8)) return rc;
  if (int rc = ensure(c, o->pr_togo, Q * K * 8)) return rc;
  if (int rc = ensure(c, o->pr_costs, Q * K * 8)) return rc;
  if (int rc = ensure(c, o->pr_sidx, Q * SC * 4)) return rc;
  if (int rc = ensure(c, o->pr_sterm, Q * SC * 8)) return rc;
  // the chain launch on a copy of the context's arguments with the source's controls and duration (traj_api.cpp build())
  const mplx_succ none{};
  mplx::PriorArgs P{};
  mplx::TrajArgs &a = P.traj;
  a.env = expand_args(c, nullptr, 0, 0, &none);
  a.env.U = src->U; a.env.nU = src->nU; a.env.udim = src->udim; a.env.dt = src->dt;
  a.starts = s->starts; a.n_starts = s->n_starts; a.start_stride = s->start_stride;
  a.actions = s->actions; a.n_traj = s->n_traj; a.action_stride = s->action_stride; a.horizon = s->horizon;
  a.yaw = (src->control & 0x10) ? 1 : 0;
  {
    const size_t H = (size_t)s->horizon, NC = 5 * D + 2;
    StageLayout l;  // (only the carving: the table is the context's own scratch, not the arena)
    const size_t o_S = l.add(Q * 4), o_n = l.add(Q * 4), o_st = l.add(Q), o_T = l.add(Q * 8), o_tau = l.add((H + 1) * Q * 8),
                 o_seg = l.add(H * NC * Q * 8);
    if (int rc = ensure(c, c->traj_tab, l.total)) return rc;
    char *base = (char *)c->traj_tab.p;
    a.tab_S = (int32_t *)(base + o_S);
    a.tab_n = (int32_t *)(base + o_n);
    a.tab_status = (uint8_t *)(base + o_st);
    a.tab_T = (double *)(base + o_T);
    a.tab_tau = (double *)(base + o_tau);
    a.tab_seg = (double *)(base + o_seg);
  }
  o->has_priors = false;  // (a failure below leaves the open set without priors ...
  HIP_TRY(c, hipMemcpyAsync(o->goals.p, o->goals0.p, Q * sizeof(mplx::PostFuse), hipMemcpyDeviceToDevice, c->stream));  // ... and with its own goals)
  HIP_TRY(c, mplx::launch_traj_chain(c->dim, src->control, a, c->stream));
  a.cost = (double *)o->pr_trav.p;
  const double B = std::ceil(c->prm.v_max * span / c->res) + 1.0;  // auto_lanes of traj_api.cpp
  HIP_TRY(c, mplx::launch_traj_traverse(c->dim, !(B > 64.0) ? 4 : B <= 256.0 ? 16 : 64, a, c->stream));
  a.cost = nullptr;
  P.dt = c->prm.dt;
  P.traverse = (const double *)o->pr_trav.p;
  P.s_idx = (int32_t *)o->pr_sidx.p; P.s_term = (double *)o->pr_sterm.p; P.costs = (double *)o->pr_costs.p;
  P.s_cap = (int64_t)SC; P.k_cap = (int64_t)K;
  P.n_steps = (int32_t *)o->pr_n.p; P.pos = (double *)o->pr_pos.p; P.togo = (double *)o->pr_togo.p; P.status = (uint8_t *)o->pr_status.p;
  P.goals0 = (const mplx::PostFuse *)o->goals0.p; P.goals = (mplx::PostFuse *)o->goals.p;
  P.goal_row = (double *)o->pr_grow.p; P.goal_hash = (uint64_t *)o->pr_ghash.p;
  HIP_TRY(c, mplx::launch_prior_build(c->dim, src->control, P, c->stream));
  o->has_priors = true;
  o->pr_cap = (int64_t)K;
  o->pr_dt = c->prm.dt;
  if (h_info && (h_info->status || h_info->n_steps)) {
    if (h_info->status) HIP_TRY(c, hipMemcpyAsync(h_info->status, o->pr_status.p, Q, hipMemcpyDeviceToHost, c->stream));
    if (h_info->n_steps) HIP_TRY(c, hipMemcpyAsync(h_info->n_steps, o->pr_n.p, Q * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return MPLX_OK;
}

int mplx_open_clear_priors(mplx_open *o) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  if (!o->has_priors) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  o->has_priors = false;
  if (o->has_goals)
    HIP_TRY(c, hipMemcpyAsync(o->goals.p, o->goals0.p, (size_t)o->Q * sizeof(mplx::PostFuse), hipMemcpyDeviceToDevice, c->stream));
  return MPLX_OK;
}

// ---- include/mplx_field.h ----------------------------------------------------------------------------------------------

int mplx_open_set_field(mplx_open *o, mplx_field *fld, const int32_t *h_field_of_query) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_set_field";
  if (!fld) return fail(c, MPLX_ERR_ARG, "%s: NULL field", who);
  if (fld->c != c) return fail(c, MPLX_ERR_ARG, "%s: the field belongs to another context", who);
  if (o->has_priors) return fail(c, MPLX_ERR_STATE, "%s: priors are in force (mplx_open_clear_priors first)", who);
  if (fld->F < 1) return fail(c, MPLX_ERR_STATE, "%s: the field is empty (mplx_field_build)", who);
  if (!o->has_goals && !c->has_goal) return fail(c, MPLX_ERR_STATE, "%s: no goal (mplx_set_goal, mplx_open_set_goals)", who);
  if (!((o->has_goals ? o->goals_vmin : c->goal_fuse.v_max) > 0)) return fail(c, MPLX_ERR_STATE, "%s: a goal field needs v_max > 0", who);
  MPLX_GUARD_BEGIN
  std::vector<int32_t> fq((size_t)o->Q);
  int32_t top = -1;
  for (int32_t q = 0; q < o->Q; q++) {
    const int32_t v = h_field_of_query ? h_field_of_query[q] : q;
    if (v < -1 || v >= fld->F) return fail(c, MPLX_ERR_ARG, "%s: query %d asks for field %d of %d", who, (int)q, (int)v, (int)fld->F);
    fq[(size_t)q] = v;
    top = std::max(top, v);
  }
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t bytes = (size_t)o->Q * 4;
  if (int rc = ensure(c, o->fld_q, bytes)) return rc;
  StageRows s;
  const auto i_q = s.in(fq.data(), bytes);
  if (int rc = stage_commit(c, &s)) return rc;
  HIP_TRY(c, hipMemcpyAsync(o->fld_q.p, s.dev<char>(i_q), bytes, hipMemcpyDeviceToDevice, c->stream));
  if (int rc = stage_fetch(c, &s)) return rc;  // (no output row: the synchronise -- fq leaves scope; the arena is free again)
  if (o->fld != fld) {
    fld->users.push_back(o);  // (first: if it throws nothing has changed)
    drop_field(o);
  }
  o->fld = fld;
  o->fld_gone = false;
  o->fld_max = top;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

int mplx_open_clear_field(mplx_open *o) {
  if (!o) return MPLX_ERR_ARG;
  drop_field(o);
  return MPLX_OK;
}

// ---- include/mplx_heur.h -----------------------------------------------------------------------------------------------

int mplx_open_set_heur(mplx_open *o, int32_t mode) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_set_heur";
  if (mode == MPLX_HEUR_REFERENCE)
    return fail(c, MPLX_ERR_ARG, "%s: MPLX_HEUR_REFERENCE is host only (the planner's mode): the device takes DEFAULT and ROBUST", who);
  if (mode != MPLX_HEUR_DEFAULT && mode != MPLX_HEUR_ROBUST) return fail(c, MPLX_ERR_ARG, "%s: unknown mode %d", who, (int)mode);
  if (mode == MPLX_HEUR_ROBUST) {
    if (o->has_priors) return fail(c, MPLX_ERR_STATE, "%s: priors are in force (mplx_open_clear_priors first)", who);
    // (a goal set later is checked by the push)
    if ((o->has_goals || c->has_goal) && !((o->has_goals ? o->goals_wmin : c->goal_fuse.w) > 0))
      return fail(c, MPLX_ERR_ARG, "%s: MPLX_HEUR_ROBUST needs w > 0", who);
  }
  o->heur_mode = mode;
  return MPLX_OK;
}

int mplx_open_prior_view_of(mplx_open *o, mplx_prior_view *v) {
  if (!o) return MPLX_ERR_ARG;
  if (!v) return fail(o->c, MPLX_ERR_ARG, "mplx_open_prior_view_of: NULL view");
  *v = mplx_prior_view{};
  if (!o->has_priors) return MPLX_OK;
  v->n_steps = (const int32_t *)o->pr_n.p;
  v->pos = (const double *)o->pr_pos.p;
  v->togo = (const double *)o->pr_togo.p;
  v->goal_row = (const double *)o->pr_grow.p;
  v->goal_hash = (const uint64_t *)o->pr_ghash.p;
  v->step_capacity = o->pr_cap;
  return MPLX_OK;
}

// ---- include/mplx_anytime.h --------------------------------------------------------------------------------------------

int mplx_open_rekey_device(mplx_open *o, double eps, int32_t write, const double *h_cut, mplx_open_bound *d_bound, mplx_open_bound *h_bound) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_rekey_device";
  if (!(eps >= 0.0) || std::isinf(eps)) return fail(c, MPLX_ERR_ARG, "%s: need a finite eps >= 0", who);
  if (h_cut)
    for (int32_t q = 0; q < o->Q; q++)
      if (!(h_cut[q] >= 0.0)) return fail(c, MPLX_ERR_ARG, "%s: cut[%d] is negative or NaN", who, (int)q);
  if (o->Q > 1 && !o->has_goals) return fail(c, MPLX_ERR_STATE, "%s: no goals (mplx_open_set_goals)", who);
  if (!o->has_goals && !c->has_goal) return fail(c, MPLX_ERR_STATE, "%s: no goal (mplx_set_goal)", who);
  MPLX_GUARD_BEGIN
  mplx::RekeyArgs r{};
  mplx::OpenArgs &a = r.o;
  if (int rc = open_args(o, who, &a)) return rc;
  a.eps = eps;
  if (int rc = heur_args(o, who, &a)) return rc;
  if (int rc = bind_device(c)) return rc;
  const size_t Q = (size_t)o->Q;
  if (int rc = ensure(c, o->rk_ctl, Q * sizeof(mplx::RekeyCtl))) return rc;
  if (!o->rk_mirror && hipHostMalloc((void **)&o->rk_mirror, std::max<size_t>(64, Q * sizeof(mplx::OpenBound)), hipHostMallocCoherent) != hipSuccess) {
    o->rk_mirror = nullptr;
    (void)hipGetLastError();
    return fail(c, MPLX_ERR_HIP, "%s: hipHostMalloc failed", who);
  }
  r.write = write ? 1 : 0;
  r.rctl = (mplx::RekeyCtl *)o->rk_ctl.p;
  r.d_bound = (mplx::OpenBound *)d_bound;
  r.mirror = o->rk_mirror;
  bool waited = false;
  if (h_cut) {
    // The cut lands in a buffer of the open set's own, not in the context's staging arena: the call holds no arena row,
    // so nothing another host-pointer call carves can move under the launch.  The wait lets the caller's array go.
    if (int rc = ensure(c, o->rk_cut, Q * 8)) return rc;
    HIP_TRY(c, hipMemcpyAsync(o->rk_cut.p, h_cut, Q * 8, hipMemcpyHostToDevice, c->stream));
    r.cut = (const double *)o->rk_cut.p;
    HIP_TRY(c, mplx::launch_open_rekey(c->dim, r, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    waited = true;
  } else {
    HIP_TRY(c, mplx::launch_open_rekey(c->dim, r, c->stream));
  }
  if (!h_bound) return MPLX_OK;
  if (!waited) HIP_TRY(c, hipStreamSynchronize(c->stream));
  table_observe(o->tab);
  if (int rc = table_open_args(o->tab, who, &c, &a)) return rc;  // a status bit: the re-key did nothing
  const volatile mplx::OpenBound *m = o->rk_mirror;
  for (int32_t q = 0; q < o->Q; q++) {
    h_bound[q].lower = m[q].lower; h_bound[q].n_open = m[q].n_open; h_bound[q].n_pruned = m[q].n_pruned; h_bound[q].n_rekeyed = m[q].n_rekeyed;
  }
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

// ---- include/mplx_best.h -----------------------------------------------------------------------------------------------

}  // extern "C"

namespace {

// Both forms: the reduce pass of the plain select, the radix select of open_best_kernel.hip, the tail of select_multi
// (whose results on a table of one query are the plain select's bytes).
int select_best(mplx_open *o, const char *who, bool single, int64_t k, double delta, const mplx_table_frontier *d_out,
                mplx_open_result *d_results, mplx_open_result *h_results) {
  mplx_ctx *c = o->c;
  if (k < 1) return fail(c, MPLX_ERR_ARG, "%s: need k >= 1", who);
  if (single && o->Q > 1) return fail(c, MPLX_ERR_STATE, "%s: the table has %d queries: mplx_open_select_best_multi_device", who, (int)o->Q);
  if (!(delta >= 0.0)) return fail(c, MPLX_ERR_ARG, "%s: need delta >= 0", who);
  if (int rc = check_frontier(c, who, d_out)) return rc;
  mplx::BestArgs b{};
  mplx::OpenArgs &a = b.o;
  if (int rc = open_args(o, who, &a)) return rc;
  if (int rc = bind_device(c)) return rc;
  const size_t bytes = mplx::best_scratch_bytes(o->Q, o->cap);
  if (int rc = ensure(c, o->best, bytes)) return rc;
  set_frontier(&a, d_out);
  a.delta = delta;
  a.result = (mplx::OpenResult *)d_results;
  a.n_tiles = (std::max<int64_t>(a.n_bound, 1) + mplx::kTableTile - 1) / mplx::kTableTile;
  const size_t Q = (size_t)o->Q;
  char *p = (char *)o->best.p;
  b.k = (uint32_t)std::min<int64_t>(k, 0x7fffffff);
  b.active = (uint32_t *)p;
  b.fin = (mplx::BestFinal *)(p + 64);
  b.fin2 = b.fin + Q;
  b.state = (mplx::BestState *)(b.fin2 + Q);
  b.hist = (uint32_t *)(b.state + (size_t)mplx::kBestPasses * Q);
  b.eqc = b.hist + (size_t)mplx::kBestPasses * Q * mplx::kBestBins;
  b.seg_stride = (int64_t)(((size_t)o->cap + mplx::kTableTile - 1) / mplx::kTableTile * (mplx::kTableTile / mplx::kBestSeg));
  HIP_TRY(c, hipMemsetAsync(o->best.p, 0, bytes, c->stream));
  HIP_TRY(c, mplx::launch_open_reduce_only(a, a.t_query != nullptr, c->stream));
  HIP_TRY(c, mplx::launch_open_best(b, c->stream));
  HIP_TRY(c, mplx::launch_open_tail_multi(a, c->stream));
  o->parity = 1 - o->parity;
  if (!h_results) return MPLX_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  table_observe(o->tab);
  if (int rc = table_open_args(o->tab, who, &c, &a)) return rc;  // a status bit: the select did nothing
  const volatile mplx::OpenResult *m = o->mirror;
  for (int32_t q = 0; q < o->Q; q++) {
    mplx_open_result *h = h_results + q;
    h->status = m[q].status; h->goal_id = m[q].goal_id; h->count = m[q].count; h->n_open = m[q].n_open;
    h->f_min = m[q].f_min; h->goal_f = m[q].goal_f; h->goal_g = m[q].goal_g;
  }
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_open_select_best_device(mplx_open *o, int64_t k, double delta, const mplx_table_frontier *d_out, mplx_open_result *d_result,
                                 mplx_open_result *h_result) {
  if (!o) return MPLX_ERR_ARG;
  MPLX_GUARD_BEGIN
  return select_best(o, "mplx_open_select_best_device", true, k, delta, d_out, d_result, h_result);
  MPLX_GUARD_END(o->c)
}

int mplx_open_select_best_multi_device(mplx_open *o, int64_t k, double delta, const mplx_table_frontier *d_out,
                                       mplx_open_result *d_results, mplx_open_result *h_results) {
  if (!o) return MPLX_ERR_ARG;
  MPLX_GUARD_BEGIN
  return select_best(o, "mplx_open_select_best_multi_device", false, k, delta, d_out, d_results, h_results);
  MPLX_GUARD_END(o->c)
}

}  // extern "C"
