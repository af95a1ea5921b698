// ray_api.cpp -- C ABI of include/mplx_ray.h: MapUtil::rayTrace over many point pairs on the map the context holds
// (ray_kernel.hip), and the ray trace of env_map::is_goal over successor lists that stay on the device.
#include "mplx_ctx.h"
#include "../../include/mplx_ray.h"

#include <algorithm>
#include <cmath>

using namespace mplx_detail;

namespace {

// Lanes per ray from a bound B on the steps that the host knows without reading device data: the smallest G of
// {4, 16, 64} with ceil(B / G) <= 4 rounds.
int auto_lanes(double bound) {
  if (!(bound > 16.0)) return 4;
  return bound <= 64.0 ? 16 : 64;
}

int check_query(mplx_ctx *c, const char *who, const double *p1, const double *p2, int64_t n, int64_t stride,
                int64_t p2_stride, int32_t lanes, const mplx_ray_out *o) {
  if (!o || !o->status || n < 0 || stride < n || (p2_stride != 0 && p2_stride < n) || (n > 0 && (!p1 || !p2)) ||
      (lanes != 0 && lanes != 4 && lanes != 16 && lanes != 64) || o->cell_cap < 0 || (o->cells && o->cell_cap == 0))
    return fail(c, MPLX_ERR_ARG, "%s: bad arguments", who);
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "%s: set the map first", who);
  if (c->n_cells > 0x7fffffffLL) return fail(c, MPLX_ERR_STATE, "%s: the map has more cells than getIndex (int32) can number", who);
  return MPLX_OK;
}

mplx::RayArgs map_args(const mplx_ctx *c) {
  mplx::RayArgs a{};
  a.map = (const int8_t *)c->map.p;
  a.dim0 = c->mdim[0]; a.dim1 = c->mdim[1]; a.dim2 = c->mdim[2];
  a.org0 = c->origin[0]; a.org1 = c->origin[1]; a.org2 = c->origin[2];
  a.res = c->res;
  return a;
}

int launch(mplx_ctx *c, const double *d_p1, const double *d_p2, int64_t n, int64_t stride, int64_t p2_stride, int32_t lanes,
           const mplx_ray_out *o) {
  mplx::RayArgs a = map_args(c);
  a.p1 = d_p1; a.p2 = d_p2; a.n = n; a.stride = stride; a.p2_stride = p2_stride;
  a.status = o->status; a.n_cells = o->n_cells; a.first_hit = o->first_hit; a.cells = o->cells; a.cell_cap = o->cell_cap;
  if (lanes == 0) {
    const int32_t longest = std::max(c->mdim[0], std::max(c->mdim[1], c->dim == 3 ? c->mdim[2] : 1));
    lanes = auto_lanes((double)longest / 0.8 + 2.0);
  }
  HIP_TRY(c, mplx::launch_ray_trace(c->dim, lanes, a, c->stream));
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_ray_trace_device(mplx_ctx *c, const double *d_p1, const double *d_p2, int64_t n, int64_t stride, int64_t p2_stride,
                          int32_t lanes, const mplx_ray_out *d_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_query(c, "mplx_ray_trace_device", d_p1, d_p2, n, stride, p2_stride, lanes, d_out)) return rc;
  if (n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  return launch(c, d_p1, d_p2, n, stride, p2_stride, lanes, d_out);
}

int mplx_ray_trace(mplx_ctx *c, const double *h_p1, const double *h_p2, int64_t n, int64_t stride, int64_t p2_stride,
                   int32_t lanes, const mplx_ray_out *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = check_query(c, "mplx_ray_trace", h_p1, h_p2, n, stride, p2_stride, lanes, h_out)) return rc;
  if (n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const int D = c->dim;
  const size_t N = (size_t)n, cell_bytes = h_out->cells ? N * (size_t)h_out->cell_cap * 4 : 0;
  // One arena block: p1 [D][n], p2 [D][n] (or D doubles), status, n_cells, first_hit, cells.  The entries of a cells row
  // past min(n_cells, cell_cap) keep the caller's bytes: they make the round trip.
  StageRows s;
  const auto i_p1 = s.in_rows(h_p1, (size_t)stride * 8, N * 8, D),
             i_p2 = p2_stride == 0 ? s.in(h_p2, (size_t)D * 8) : s.in_rows(h_p2, (size_t)p2_stride * 8, N * 8, D),
             o_status = s.out_or_scratch(h_out->status, N), o_count = s.out(h_out->n_cells, N * 4), o_hit = s.out(h_out->first_hit, N * 4),
             o_cells = s.inout(h_out->cells, cell_bytes);
  if (lanes == 0) {
    // the points are at hand here: the longest ray's own step count instead of the map's bound (BAD rays trace nothing)
    double steps = 0.0;
    for (int64_t k = 0; k < n; k++) {
      double linf = 0.0;
      for (int i = 0; i < D; i++) {
        const double q = std::fabs((h_p2[p2_stride == 0 ? (int64_t)i : (int64_t)i * p2_stride + k] - h_p1[(int64_t)i * stride + k]) / c->res);
        linf = q > linf ? q : linf;  // (a NaN never becomes the maximum)
      }
      const double md = linf / 0.8;
      if (md < 2147483648.0 && md > steps) steps = md;
    }
    lanes = auto_lanes(steps);
  }
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_ray_out d{};
  d.status = s.dev<uint8_t>(o_status);
  d.n_cells = s.dev<int32_t>(o_count);
  d.first_hit = s.dev<int32_t>(o_hit);
  d.cells = s.dev<int32_t>(o_cells);
  d.cell_cap = h_out->cell_cap;
  if (int rc = launch(c, s.dev<double>(i_p1), s.dev<double>(i_p2), n, n, p2_stride == 0 ? 0 : n, lanes, &d)) return rc;
  return stage_fetch(c, &s);
}

// goal_or_null / the context's goal, or (d_goals != null) the goal per list entry
static int goal_sight(mplx_ctx *c, const mplx_succ_lists *d_lists, int64_t n_nodes, const mplx_goal_spec *goal, const int32_t *d_row_query,
                      const mplx::PostFuse *d_goals, double goals_tol, uint8_t *d_flags) {
  if (!d_lists || n_nodes < 0 || !d_flags || !d_lists->count || !d_lists->state || (goal && !goal->goal) || (d_goals && !d_row_query))
    return fail(c, MPLX_ERR_ARG, "mplx_goal_sight_device: the lists need count and state, and a flags row");
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "mplx_goal_sight_device: set the map first");
  if (!d_goals && !goal && !c->has_goal) return fail(c, MPLX_ERR_STATE, "mplx_goal_sight_device: no goal (mplx_set_goal or goal_or_null)");
  if (c->n_cells > 0x7fffffffLL)
    return fail(c, MPLX_ERR_STATE, "mplx_goal_sight_device: the map has more cells than getIndex (int32) can number");
  if (!d_lists->node_stride && !c->has_U) return fail(c, MPLX_ERR_STATE, "mplx_goal_sight_device: controls not set");
  if (n_nodes == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // yaw pinning: the lists must be final
  const int64_t S = list_stride(c, d_lists), total = n_nodes * S;
  if (total >= 0x7f7f7f7fLL)
    return fail(c, MPLX_ERR_ARG, "mplx_goal_sight_device: %lld list entries exceed the int32 index", (long long)total);
  // worklist: the count word on a line of its own, then one index per slot (every slot may be a candidate)
  if (int rc = ensure(c, c->ray_work, 256 + (size_t)total * 4)) return rc;
  HIP_TRY(c, hipMemsetAsync(c->ray_work.p, 0, 4, c->stream));
  mplx::GoalSightArgs a{};
  a.ray = map_args(c);
  a.count = d_lists->count;
  a.state = d_lists->state;
  a.n_nodes = n_nodes;
  a.nstride = S;
  a.sstride = d_lists->state_stride;
  if (d_goals) {
    a.goals = d_goals;
    a.row_query = d_row_query;
  } else {
    const double *g = goal ? goal->goal : c->goal_fuse.goal;
    for (int i = 0; i < c->dim; i++) a.goal[i] = g[i];
  }
  a.flags = d_flags;
  a.work_count = (uint32_t *)c->ray_work.p;
  a.work = (int32_t *)((char *)c->ray_work.p + 256);
  // a candidate lies within tol_pos of the goal on every axis: at most tol_pos / res / 0.8 steps
  const double tol = d_goals ? goals_tol : goal ? goal->tol_pos : c->goal_fuse.tol_pos;
  HIP_TRY(c, mplx::launch_goal_sight(c->dim, auto_lanes(tol / c->res / 0.8), c->n_cus, a, c->stream));
  return MPLX_OK;
}

int mplx_goal_sight_device(mplx_ctx *c, const mplx_succ_lists *d_lists, int64_t n_nodes, const mplx_goal_spec *goal,
                           uint8_t *d_flags) {
  if (!c) return MPLX_ERR_ARG;
  return goal_sight(c, d_lists, n_nodes, goal, nullptr, nullptr, 0.0, d_flags);
}

}  // extern "C"

int mplx_detail::goal_sight_rows(mplx_ctx *c, const mplx_succ_lists *d_lists, int64_t n_nodes, const int32_t *d_row_query,
                                 const mplx::PostFuse *d_goals, double tol, uint8_t *d_flags) {
  if (!d_goals) return fail(c, MPLX_ERR_ARG, "goal_sight_rows: NULL goals");
  return goal_sight(c, d_lists, n_nodes, nullptr, d_row_query, d_goals, tol, d_flags);
}
