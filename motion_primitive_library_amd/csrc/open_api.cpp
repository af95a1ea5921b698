// open_api.cpp -- C ABI of include/mplx_open.h: the open set of a node table (open_kernel.hip).  The open set's arrays,
// control blocks and scratch are its own; launches go to the stream of the table's context.  No call touches the
// staging arena: push and select take device pointers only.
#include "mplx_ctx.h"
#include "../../include/mplx_open.h"
#include "../../include/mplx_ray.h"

#include <algorithm>
#include <cmath>

using namespace mplx_detail;

static_assert(sizeof(mplx::OpenResult) == sizeof(mplx_open_result), "mplx::OpenResult is mplx_open_result");

struct mplx_open {
  mplx_table *tab = nullptr;
  mplx_ctx *c = nullptr;
  int64_t cap = 0;
  DevBuf f, flags, ctl, mark, tot;
  DevBuf rows;                          // push with the ray trace: per row a flags byte and a count; grows on demand
  mplx::OpenResult *mirror = nullptr;   // pinned
  int parity = 0;                       // which control block the next select reduces into
};

namespace {

void release_open(mplx_open *o) {
  for (DevBuf *b : {&o->f, &o->flags, &o->ctl, &o->mark, &o->tot, &o->rows}) release(*b);
  if (o->mirror) (void)hipHostFree(o->mirror);
  delete o;
}

// the table's fields (MPLX_ERR_STATE for a table with a status bit) and the open set's own
int open_args(mplx_open *o, const char *who, mplx::OpenArgs *a) {
  mplx_ctx *c = nullptr;
  if (int rc = table_open_args(o->tab, who, &c, a)) return rc;
  a->f = (unsigned long long *)o->f.p;
  a->flags = (uint8_t *)o->flags.p;
  a->ctl = (mplx::OpenCtl *)o->ctl.p + o->parity;
  a->ctl_next = (mplx::OpenCtl *)o->ctl.p + (1 - o->parity);
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
  const size_t cap = (size_t)a.cap, tiles = (cap + mplx::kTableTile - 1) / mplx::kTableTile;
  if (!rc) rc = ensure(c, o->f, cap * 8);
  if (!rc) rc = ensure(c, o->flags, cap);
  if (!rc) rc = ensure(c, o->ctl, 2 * sizeof(mplx::OpenCtl));
  if (!rc) rc = ensure(c, o->mark, cap);
  if (!rc) rc = ensure(c, o->tot, tiles * 4);
  if (!rc && hipHostMalloc((void **)&o->mirror, 64, hipHostMallocCoherent) != hipSuccess)
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
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_push_device";
  if (n_max < 0 || !(eps >= 0.0) || std::isinf(eps)) return fail(c, MPLX_ERR_ARG, "%s: need n_max >= 0 and a finite eps >= 0", who);
  if (int rc = check_frontier(c, who, d_rows)) return rc;
  if (!c->has_goal) return fail(c, MPLX_ERR_STATE, "%s: no goal (mplx_set_goal)", who);
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
  if (!sight) {
    HIP_TRY(c, mplx::launch_open_push(c->dim, 0, a, rows, c->stream));
    return MPLX_OK;
  }
  // around the goal passes of ray_kernel.hip: the frontier as `rows` lists of stride 1 with a flags byte each
  const size_t o_cnt = align256((size_t)rows);
  if (int rc = ensure(c, o->rows, o_cnt + (size_t)rows * 4)) return rc;
  a.row_flags = (uint8_t *)o->rows.p;
  a.row_count = (int32_t *)((char *)o->rows.p + o_cnt);
  HIP_TRY(c, mplx::launch_open_push(c->dim, 0, a, rows, c->stream));
  mplx_succ_lists L{};
  L.count = a.row_count;
  L.state = d_rows->state;
  L.state_stride = d_rows->state_stride;
  L.node_stride = 1;
  if (int rc = mplx_goal_sight_device(c, &L, rows, nullptr, a.row_flags)) return rc;
  HIP_TRY(c, mplx::launch_open_push(c->dim, 1, a, rows, c->stream));
  return MPLX_OK;
}

int mplx_open_select_device(mplx_open *o, double delta, const mplx_table_frontier *d_out, mplx_open_result *d_result,
                            mplx_open_result *h_result) {
  if (!o) return MPLX_ERR_ARG;
  mplx_ctx *c = o->c;
  const char *who = "mplx_open_select_device";
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

}  // extern "C"
