// wait_api.cpp -- C ABI of include/mplx_wait.h: the zero control's entry appended to the successor lists of an expansion
// (wait_kernel.hip).  Device pointers only; one asynchronous launch on the context's stream.
#include "mplx_ctx.h"
#include "../../include/mplx_wait.h"

using namespace mplx_detail;

namespace {

constexpr int64_t kMaxEntries = 0x7ffffffeLL;  // as the node table's relax

}  // namespace

// the smallest row of the control table whose every entry is == 0.0 (-0.0 counts), or -1
int32_t mplx_detail::zero_action(const mplx_ctx *c) {
  for (int32_t a = 0; a < c->nU; a++) {
    bool zero = true;
    for (int32_t j = 0; j < c->udim && zero; j++) zero = c->h_U[(size_t)a * c->udim + j] == 0.0;
    if (zero) return a;
  }
  return -1;
}

extern "C" int mplx_lists_add_wait_device(mplx_ctx *c, const mplx_succ_lists *L, int64_t n_nodes, const double *d_parent_state,
                                          int64_t parent_stride, const int32_t *d_parent_id, int64_t *d_n_added) {
  if (!c) return MPLX_ERR_ARG;
  const char *who = "mplx_lists_add_wait_device";
  if (!L || n_nodes < 0 || !d_parent_state) return fail(c, MPLX_ERR_ARG, "%s: NULL argument or n_nodes < 0", who);
  if (!L->count || !L->action || !L->cost) return fail(c, MPLX_ERR_ARG, "%s: the lists need count, action and cost", who);
  const int64_t S = list_stride(c, L);
  if (S < 1 || n_nodes > kMaxEntries / S) return fail(c, MPLX_ERR_ARG, "%s: node_stride < 1 or more than 2^31 - 2 list entries", who);
  if (parent_stride < n_nodes) return fail(c, MPLX_ERR_ARG, "%s: parent_stride < n_nodes", who);
  if (L->state && L->state_stride < n_nodes * S) return fail(c, MPLX_ERR_ARG, "%s: state_stride < n_nodes * node_stride", who);
  if (!c->has_params) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_params has not been called", who);
  if (!c->has_U) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_controls has not been called", who);
  const int need = c->dim + ((c->prm.control & 0x10) ? 1 : 0);
  if (c->udim < need)
    return fail(c, MPLX_ERR_STATE, "%s: controls have %d entries per row, control flag 0x%x needs %d", who, c->udim, c->prm.control, need);
  if ((L->heur || L->flags) && !c->has_goal) return fail(c, MPLX_ERR_STATE, "%s: heur / flags need mplx_set_goal", who);
  const int32_t a0 = zero_action(c);
  if (a0 < 0) return fail(c, MPLX_ERR_STATE, "%s: the control table has no all-zero row: there is no wait action", who);
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // yaw pinning: the lists must be final
  if (n_nodes == 0) return MPLX_OK;
  const mplx_succ none{};
  mplx::WaitArgs a{};
  a.env = expand_args(c, nullptr, 0, 0, &none);
  a.a0 = a0;
  a.count = L->count; a.action = L->action; a.cost = L->cost; a.hash = L->hash;
  a.state = L->state; a.state_stride = L->state_stride; a.iters = L->iters;
  a.n_rows = n_nodes; a.S = S;
  a.parent_id = d_parent_id; a.parent_state = d_parent_state; a.parent_stride = parent_stride;
  a.post = c->goal_fuse;
  a.post.heur = L->heur;
  a.post.flags = L->flags;
  a.n_added = (unsigned long long *)d_n_added;
  HIP_TRY(c, mplx::launch_lists_add_wait(c->dim, c->prm.control, a, c->stream));
  return MPLX_OK;
  MPLX_GUARD_END(c)
}
