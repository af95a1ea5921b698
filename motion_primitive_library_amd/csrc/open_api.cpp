// open_api.cpp -- C ABI of include/mplx_open.h: the open set of a node table (open_kernel.hip).  The open set's arrays,
// control blocks and scratch are its own; launches go to the stream of the table's context.  No call touches the
// staging arena: push and select take device pointers only.
#include "mplx_ctx.h"
#include "../../include/mplx_multi.h"
#include "../../include/mplx_ray.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace mplx_detail;

static_assert(sizeof(mplx::OpenResult) == sizeof(mplx_open_result), "mplx::OpenResult is mplx_open_result");

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
};

namespace {

void release_open(mplx_open *o) {
  for (DevBuf *b : {&o->f, &o->flags, &o->ctl, &o->mark, &o->tot, &o->rows, &o->goals}) release(*b);
  if (o->mirror) (void)hipHostFree(o->mirror);
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
  a.goal = c->goal_fuse;
  a.goals = o->has_goals ? (const mplx::PostFuse *)o->goals.p : nullptr;
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
  double tol = 0.0;
  for (int32_t q = 0; q < n; q++) {
    if (int rc = goal_fuse_of(c, who, &h_goals[q], &f[(size_t)q])) return rc;
    tol = std::max(tol, f[(size_t)q].tol_pos);
  }
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t bytes = (size_t)n * sizeof(mplx::PostFuse);
  if (int rc = ensure(c, o->goals, bytes)) return rc;
  StageLayout l;
  const size_t o_g = l.add(bytes);
  if (int rc = stage_commit(c, &l)) return rc;
  HIP_TRY(c, stage_in(c, l.base + o_g, f.data(), bytes));
  HIP_TRY(c, hipMemcpyAsync(o->goals.p, l.base + o_g, bytes, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (f leaves scope; the arena is free again)
  o->has_goals = true;
  o->goals_tol = tol;
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

}  // extern "C"
