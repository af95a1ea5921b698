// replan_api.cpp -- C ABI of include/mplx_replan.h: the rebase of a node table after a map edit (replan_kernel.hip) and
// the closed push of its open set (open_kernel.hip).  The passes' scratch is the table's own; launches go to the stream
// of the table's context.  No call touches the staging arena: all three take device pointers only.
#include "mplx_ctx.h"
#include "../../include/mplx_replan_timed.h"

#include <algorithm>

using namespace mplx_detail;

static_assert(sizeof(mplx::ReplanResult) == sizeof(mplx_rebase_result), "mplx::ReplanResult is mplx_rebase_result");

namespace {

// passes of pointer doubling that decide every chain of a table with at most `bound` nodes: ceil(log2(bound)) + 1
int resolve_passes(int64_t bound) {
  int p = 0;
  while ((1LL << p) < std::max<int64_t>(bound, 2)) p++;
  return p + 1;
}

// what mplx_table_rebase_timed_device adds to a rebase
struct Timed {
  int32_t allow_wait;
  mplx_reserve *res;
  int64_t *d_hit, *d_n_blocked;
};

// d_roots null: the plain call with root_id; timed null: the untimed rebases, whose launches are what they were
int rebase(mplx_table *t, const char *who, int32_t root_id, const int32_t *d_roots, int32_t check_edges, const mplx_table_frontier *f,
           mplx_rebase_result *d_result, mplx_rebase_result *h_result, const Timed *timed = nullptr) {
  mplx::ReplanArgs a{};
  mplx_ctx *c = nullptr;
  int32_t time_keys = 0;
  const int usable = table_replan_args(t, who, false, &c, &a, timed ? &time_keys : nullptr);  // (sets c whatever it answers)
  // the multi rebase's own checks first, in its order: the frontier, then the table's state
  if (!f || !f->id || !f->g || !f->state || !f->count || f->capacity < 0 || f->state_stride < f->capacity)
    return fail(c, MPLX_ERR_ARG, "%s: the frontier needs id, g, state and count, and state_stride >= capacity >= 0", who);
  if (usable) return usable;
  mplx::ReplanTimedArgs ta{};
  if (timed && timed->res) {
    mplx_ctx *rc_ctx = nullptr;
    const int rrc = reserve_table_args(timed->res, who, &rc_ctx, &ta.res);  // (sets rc_ctx whatever it answers)
    if (rc_ctx != c) return fail(c, MPLX_ERR_ARG, "%s: the reservation table belongs to another context", who);
    if (rrc) return rrc;
    if (ta.res.Q != a.n_queries) return fail(c, MPLX_ERR_ARG, "%s: %d queries were set, the table has %d", who, (int)ta.res.Q, (int)a.n_queries);
    if (!c->has_params) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_params has not been called", who);
    if (!c->has_U) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_controls has not been called", who);
    ta.use_res = 1;
  }
  if (check_edges)
    if (int rc = ctx_ready(c)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (timed)
    if (int rc = resolve_pending(c)) return rc;  // yaw pinning: decisions still pending are final first, as the check has it
  if (a.n_bound == 0) {  // a table without nodes
    HIP_TRY(c, hipMemsetAsync(f->count, 0, 8, c->stream));
    if (d_result) HIP_TRY(c, hipMemsetAsync(d_result, 0, sizeof *d_result, c->stream));
    if (h_result) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      table_observe(t);
      *h_result = mplx_rebase_result{0, 0, 0};
    }
    return MPLX_OK;
  }
  if (int rc = table_replan_args(t, who, true, &c, &a, timed ? &time_keys : nullptr)) return rc;
  if (check_edges) {
    const mplx_succ none{};
    a.env = expand_args(c, nullptr, 0, 0, &none);
    // the band of the yaw pinning (margin, the exact-tie exemption), as a rollout takes it: nothing is recorded per
    // node and nothing becomes pending -- an edge inside the band is simply bad
    if (int rc = yaw_slot(c, &a.env.yaw)) return rc;
    a.band = a.env.yaw.amb ? 1 : 0;
    a.env.yaw.amb = nullptr;
    a.env.yaw.any_host = nullptr;
  }
  a.check_edges = check_edges ? 1 : 0;
  a.root_id = root_id;
  a.root_of_query = d_roots;
  a.n_tiles = (a.n_bound + mplx::kTableTile - 1) / mplx::kTableTile;
  a.f_id = f->id; a.f_g = f->g; a.f_state = f->state; a.f_stride = f->state_stride; a.f_cap = f->capacity; a.f_count = f->count;
  if (!timed) {
    HIP_TRY(c, mplx::launch_replan_rebase(c->dim, c->prm.control, a, resolve_passes(a.n_bound), c->stream));
  } else {
    ta.R = a;
    ta.time_keys = time_keys;
    ta.allow_wait = timed->allow_wait ? 1 : 0;
    ta.a0 = c->has_U ? zero_action(c) : -1;
    if (ta.use_res) {
      ta.res.node_query = a.n_queries > 1 ? a.query : nullptr;
      ta.res.node_cap = a.cap;
      ta.hit = (long long *)timed->d_hit;
      ta.n_blocked = (unsigned long long *)timed->d_n_blocked;
    }
    HIP_TRY(c, mplx::launch_replan_rebase_timed(c->dim, c->prm.control, ta, resolve_passes(a.n_bound), c->stream));
  }
  if (d_result) HIP_TRY(c, hipMemcpyAsync(d_result, a.counters, sizeof *d_result, hipMemcpyDeviceToDevice, c->stream));
  if (!h_result) return MPLX_OK;
  HIP_TRY(c, hipMemcpyAsync(h_result, a.counters, sizeof *h_result, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  table_observe(t);
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_table_rebase_device(mplx_table *t, int32_t root_id, int32_t check_edges, const mplx_table_frontier *d_kept,
                             mplx_rebase_result *d_result, mplx_rebase_result *h_result) {
  if (!t) return MPLX_ERR_ARG;
  const char *who = "mplx_table_rebase_device";
  mplx::ReplanArgs a{};
  mplx_ctx *c = nullptr;
  const int usable = table_replan_args(t, who, false, &c, &a);
  if (root_id < -1) return fail(c, MPLX_ERR_ARG, "%s: root_id = %d (a node id, or -1 for the seeds)", who, (int)root_id);
  if (!usable && a.n_queries > 1)
    return fail(c, MPLX_ERR_STATE, "%s: the table has %d queries: mplx_table_rebase_multi_device", who, (int)a.n_queries);
  return rebase(t, who, root_id, nullptr, check_edges, d_kept, d_result, h_result);
}

int mplx_table_rebase_multi_device(mplx_table *t, const int32_t *d_root_of_query, int32_t check_edges, const mplx_table_frontier *d_kept,
                                   mplx_rebase_result *d_result, mplx_rebase_result *h_result) {
  if (!t) return MPLX_ERR_ARG;
  const char *who = "mplx_table_rebase_multi_device";
  if (!d_root_of_query) {
    mplx::ReplanArgs a{};
    mplx_ctx *c = nullptr;
    (void)table_replan_args(t, who, false, &c, &a);
    return fail(c, MPLX_ERR_ARG, "%s: NULL d_root_of_query", who);
  }
  return rebase(t, who, -1, d_root_of_query, check_edges, d_kept, d_result, h_result);
}

int mplx_table_rebase_timed_device(mplx_table *t, const int32_t *d_root_of_query, int32_t check_edges, int32_t allow_wait,
                                   mplx_reserve *res, const mplx_table_frontier *d_kept, int64_t *d_hit, int64_t *d_n_blocked,
                                   mplx_rebase_result *d_result, mplx_rebase_result *h_result) {
  if (!t) return MPLX_ERR_ARG;
  const char *who = "mplx_table_rebase_timed_device";
  if (!d_root_of_query) {
    mplx::ReplanArgs a{};
    mplx_ctx *c = nullptr;
    int32_t tk = 0;
    (void)table_replan_args(t, who, false, &c, &a, &tk);
    return fail(c, MPLX_ERR_ARG, "%s: NULL d_root_of_query", who);
  }
  const Timed timed{allow_wait, res, d_hit, d_n_blocked};
  return rebase(t, who, -1, d_root_of_query, check_edges, d_kept, d_result, h_result, &timed);
}

int mplx_open_push_closed_device(mplx_open *o, const mplx_table_frontier *d_rows, int64_t n_max, double eps, int32_t sight) {
  if (!o) return MPLX_ERR_ARG;
  return open_push(o, "mplx_open_push_closed_device", d_rows, n_max, eps, sight, true);
}

}  // extern "C"
