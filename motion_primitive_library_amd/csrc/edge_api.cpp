// edge_api.cpp -- C ABI of the batched edge re-validation (edge_kernel.hip).
#include "mplx_ctx.h"

using namespace mplx_detail;

extern "C" int mplx_check_edges(mplx_ctx *c, const double *h_parents, const int32_t *h_actions, int64_t n_edges,
                                int64_t stride, const mplx_edges_out *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (!h_out || n_edges < 0 || stride < n_edges || ((!h_parents || !h_actions) && n_edges > 0))
    return fail(c, MPLX_ERR_ARG, "mplx_check_edges: bad arguments");
  if (h_out->cells && (h_out->cell_cap <= 0 || !h_out->cell_count))
    return fail(c, MPLX_ERR_ARG, "mplx_check_edges: cells need cell_cap > 0 and cell_count");
  if (!c->has_map || !c->has_params || !c->has_U) return fail(c, MPLX_ERR_STATE, "mplx_check_edges: map, params and controls must be set");
  if (n_edges == 0) return MPLX_OK;
  for (int64_t e = 0; e < n_edges; e++)
    if (h_actions[e] < 0 || h_actions[e] >= c->nU)
      return fail(c, MPLX_ERR_ARG, "mplx_check_edges: action %d of edge %lld is outside the control table", h_actions[e], (long long)e);
  if (int rc = bind_device(c)) return rc;
  const int F = 4 * c->dim + 2;
  const size_t n = (size_t)n_edges, cell_bytes = h_out->cells ? n * (size_t)h_out->cell_cap * 4 : 0;
  StageRows s;
  const auto i_parents = s.in_rows(h_parents, (size_t)stride * 8, n * 8, F), i_action = s.in(h_actions, n * 4),
             o_free = s.out(h_out->free_flag, n), o_outside = s.out(h_out->outside, n), o_cost = s.out(h_out->cost, n * 8),
             o_count = s.out(h_out->cell_count, n * 4), o_cells = s.out(h_out->cells, cell_bytes);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx::EdgeArgs a{};
  a.map = (const int8_t *)c->map.p;
  a.region = c->has_region ? (const uint32_t *)c->region_bits.p : nullptr;
  a.dim0 = c->mdim[0]; a.dim1 = c->mdim[1]; a.dim2 = c->mdim[2];
  a.org0 = c->origin[0]; a.org1 = c->origin[1]; a.org2 = c->origin[2];
  a.res = c->res;
  a.dt = c->prm.dt; a.w = c->prm.w;
  a.U = (const double *)c->U.p;
  a.nU = c->nU; a.udim = c->udim;
  a.parents = s.dev<double>(i_parents);
  a.action = s.dev<int32_t>(i_action);
  a.n_edges = n_edges; a.stride = n_edges;
  a.free_out = s.dev<uint8_t>(o_free); a.outside_out = s.dev<uint8_t>(o_outside); a.cost = s.dev<double>(o_cost);
  a.cell_count = s.dev<int32_t>(o_count);
  if (h_out->cells) { a.cells = s.dev<int32_t>(o_cells); a.cell_cap = h_out->cell_cap; }
  HIP_TRY(c, mplx::launch_check_edges(c->dim, c->prm.control, a, c->stream));
  return stage_fetch(c, &s);
}
