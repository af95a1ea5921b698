// body_api.cpp -- C ABI of include/mplx_body.h: the ellipsoid body, its point cloud binned on the device and the checks of
// successor lists and of trajectory sets against it (body_kernel.hip).  The points, their grid and the grid's header
// are the mplx_body's own memory; launches go to the context's stream; the host-pointer twin of the set check copies
// its [K] rows through a row buffer the body owns (not the context's staging arena).
#include "mplx_body_args.h"
#include "mplx_poly.h"
#include "../../include/mplx_body.h"
#include "../../include/mplx_map_util.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

using namespace mplx_detail;

struct mplx_body {
  mplx_ctx *c = nullptr;
  bool has_shape = false, filled = false, binned = false;
  mplx::BodyShape sh{};
  double edge_auto = 0;
  int cell_mult = 1;  // MPLX_BODY_CELL_MULT
  int64_t n = 0, generation = 0;
  DevBuf raw;    // [n][D]: the points as they were given
  DevBuf pts;    // [D][n] cell-contiguous
  DevBuf idx;    // [n] original index per slot
  DevBuf cop;    // [n] cell of point
  DevBuf cells;  // [kBodyMaxCells + 1]
  DevBuf hdr;    // BodyGrid, then BodyBox
  DevBuf rows;   // the host twin of the set check: hit [K], n_hit, status [K]
};

namespace {

constexpr int64_t kMaxEntries = 0x7ffffffeLL;  // as the node table's relax
constexpr size_t kBoxAt = 256;                 // offset of the BodyBox in hdr

// bins the kept points with the shape in force (needs both)
int bin(mplx_body *b) {
  mplx_ctx *c = b->c;
  b->binned = false;
  if (!b->has_shape || !b->filled) return MPLX_OK;
  const size_t n = (size_t)b->n, D = (size_t)c->dim;
  if (int rc = ensure(c, b->pts, std::max<size_t>(n * D * 8, 256))) return rc;
  if (int rc = ensure(c, b->idx, std::max<size_t>(n * 4, 256))) return rc;
  if (int rc = ensure(c, b->cop, std::max<size_t>(n * 4, 256))) return rc;
  if (int rc = ensure(c, b->cells, ((size_t)mplx::kBodyMaxCells + 1) * 4)) return rc;
  if (int rc = ensure(c, b->hdr, 512)) return rc;
  mplx::BodyBuildArgs a{};
  a.xyz = (const double *)b->raw.p;
  a.n = b->n;
  a.edge0 = b->edge_auto * (double)b->cell_mult;
  a.grid = (mplx::BodyGrid *)b->hdr.p;
  a.box = (mplx::BodyBox *)((char *)b->hdr.p + kBoxAt);
  a.cell_of_point = (int32_t *)b->cop.p;
  a.cell_start = (int32_t *)b->cells.p;
  a.pts = (double *)b->pts.p;
  a.idx = (int32_t *)b->idx.p;
  HIP_TRY(c, mplx::launch_body_build(c->dim, a, c->stream));
  b->binned = true;
  return MPLX_OK;
}

int check_n(mplx_body *b, const char *who, int64_t n) {
  mplx_ctx *c = b->c;
  if (n < 0) return fail(c, MPLX_ERR_ARG, "%s: n < 0", who);
  if (n > 0x7ffffffeLL || n > (int64_t)MPLX_BODY_MAX_BYTES / (8 * (int64_t)c->dim))
    return fail(c, MPLX_ERR_ARG, "%s: %lld points exceed MPLX_BODY_MAX_BYTES or 2^31 - 2", who, (long long)n);
  return MPLX_OK;
}

int begin_fill(mplx_body *b, int64_t n) {
  b->filled = b->binned = false;
  return ensure(b->c, b->raw, std::max<size_t>((size_t)n * (size_t)b->c->dim * 8, 256));
}

int end_fill(mplx_body *b, int64_t n) {
  b->n = n;
  b->filled = true;
  b->generation++;
  return bin(b);
}

int ready(mplx_body *b, const char *who) {
  if (!b->has_shape) return fail(b->c, MPLX_ERR_STATE, "%s: mplx_body_set_shape has not been called", who);
  if (!b->filled || !b->binned) return fail(b->c, MPLX_ERR_STATE, "%s: the cloud has not been filled", who);
  return MPLX_OK;
}

mplx::BodyCloud cloud_of(const mplx_body *b) {
  mplx::BodyCloud cl{};
  cl.grid = (const mplx::BodyGrid *)b->hdr.p;
  cl.cell_start = (const int32_t *)b->cells.p;
  cl.pts = (const double *)b->pts.p;
  cl.idx = (const int32_t *)b->idx.p;
  cl.n = b->n;
  return cl;
}

int check_poly_args(mplx_body *b, mplx_poly *p, const char *who, const mplx_body_poly_in *in, const mplx_body_poly_out *out) {
  mplx_ctx *c = b->c;
  if (!p) return fail(c, MPLX_ERR_ARG, "%s: NULL poly", who);
  if (p->c != c) return fail(c, MPLX_ERR_ARG, "%s: the poly belongs to another context", who);
  if (!in || !out) return fail(c, MPLX_ERR_ARG, "%s: NULL in / out", who);
  if (!(in->step > 0) || !std::isfinite(in->step)) return fail(c, MPLX_ERR_ARG, "%s: step must be > 0 and finite", who);
  if (int rc = ready(b, who)) return rc;
  if (!p->solved) return fail(c, MPLX_ERR_STATE, "%s: nothing has been solved or loaded into this poly", who);
  return MPLX_OK;
}

int poly_launch(mplx_body *b, mplx_poly *p, double step, int64_t *d_hit, uint8_t *d_status, int64_t *d_n_hit) {
  mplx_ctx *c = b->c;
  mplx::BodyPolyArgs a{};
  a.shape = b->sh;
  a.cloud = cloud_of(b);
  a.traj = poly_table_args(p);
  a.K = p->n;
  a.step = step;
  a.hit = (long long *)d_hit; a.status = d_status; a.n_hit = (unsigned long long *)d_n_hit;
  HIP_TRY(c, mplx::launch_body_check_poly(c->dim, a, c->stream));
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_body_create(mplx_ctx *c, mplx_body **out) {
  if (!c) return MPLX_ERR_ARG;
  if (!out) return fail(c, MPLX_ERR_ARG, "mplx_body_create: NULL out");
  *out = nullptr;
  MPLX_GUARD_BEGIN
  mplx_body *b = new mplx_body;
  b->c = c;
  if (const char *e = std::getenv("MPLX_BODY_CELL_MULT")) {
    const int m = std::atoi(e);
    if (m >= 1 && m <= 1024) b->cell_mult = m;
  }
  *out = b;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

void mplx_body_destroy(mplx_body *b) {
  if (!b) return;
  (void)hipSetDevice(b->c->device);
  (void)hipStreamSynchronize(b->c->stream);
  for (DevBuf *d : {&b->raw, &b->pts, &b->idx, &b->cop, &b->cells, &b->hdr, &b->rows}) release(*d);
  delete b;
}

int mplx_body_set_shape(mplx_body *b, double r, double h, double g, double min_cos_tilt) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  const char *who = "mplx_body_set_shape";
  if (!std::isfinite(r) || !(r > 0) || !std::isfinite(h) || !(h > 0)) return fail(c, MPLX_ERR_ARG, "%s: r and h must be finite and > 0", who);
  if (!std::isfinite(g) || !(g > 0)) return fail(c, MPLX_ERR_ARG, "%s: g must be finite and > 0", who);
  if (!(min_cos_tilt >= 0) || !(min_cos_tilt < 1)) return fail(c, MPLX_ERR_ARG, "%s: min_cos_tilt must lie in [0, 1)", who);
  const double R = std::max(r, h);
  const double RR = (R * R) * 1.0000001;
  if (!std::isfinite(RR) || !(r * r > 0) || !(h * h > 0)) return fail(c, MPLX_ERR_ARG, "%s: r or h out of range", who);
  if (int rc = bind_device(c)) return rc;
  b->sh.g = g; b->sh.rr = r * r; b->sh.hh = h * h; b->sh.RR = RR; b->sh.mct2 = min_cos_tilt * min_cos_tilt;
  b->edge_auto = std::sqrt(RR) * 1.000001;  // a hair above sqrt(RR): DESIGN.md 4.29
  b->has_shape = true;
  return bin(b);
}

int mplx_body_fill(mplx_body *b, const double *h_xyz, int64_t n) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  const char *who = "mplx_body_fill";
  if (int rc = check_n(b, who, n)) return rc;
  if (n > 0 && !h_xyz) return fail(c, MPLX_ERR_ARG, "%s: NULL points", who);
  if (int rc = bind_device(c)) return rc;
  if (int rc = begin_fill(b, n)) return rc;
  if (n > 0) HIP_TRY(c, hipMemcpyAsync(b->raw.p, h_xyz, (size_t)n * (size_t)c->dim * 8, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int rc = end_fill(b, n)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

int mplx_body_fill_device(mplx_body *b, const double *d_xyz, int64_t n) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  const char *who = "mplx_body_fill_device";
  if (int rc = check_n(b, who, n)) return rc;
  if (n > 0 && !d_xyz) return fail(c, MPLX_ERR_ARG, "%s: NULL points", who);
  if (int rc = bind_device(c)) return rc;
  if (int rc = begin_fill(b, n)) return rc;
  if (n > 0) HIP_TRY(c, hipMemcpyAsync(b->raw.p, d_xyz, (size_t)n * (size_t)c->dim * 8, hipMemcpyDeviceToDevice, c->stream));
  return end_fill(b, n);
}

int mplx_body_fill_map(mplx_body *b, int kind) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  const char *who = "mplx_body_fill_map";
  if (kind != MPLX_CELL_OCCUPIED && kind != MPLX_CELL_FREE && kind != MPLX_CELL_UNKNOWN) return fail(c, MPLX_ERR_ARG, "%s: bad kind", who);
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "%s: set the map first", who);
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  // the count and scan launches of mplx_map_cloud, then its fill launch straight into the body's own rows
  const int D = c->dim;
  const int64_t n_col = (int64_t)c->mdim[0] * (D == 3 ? c->mdim[1] : 1);
  const size_t count_bytes = align256((size_t)n_col * 4);
  if (int rc = ensure(c, c->prep_b, count_bytes + (size_t)(n_col + 1) * 8)) return rc;
  int32_t *count = (int32_t *)c->prep_b.p;
  int64_t *offs = (int64_t *)((char *)c->prep_b.p + count_bytes);
  HIP_TRY(c, mplx::launch_cloud_count((const int8_t *)c->map.p, D, c->mdim, kind, count, offs, c->stream));
  int64_t total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, offs + n_col, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (int rc = check_n(b, who, total)) return rc;
  if (int rc = begin_fill(b, total)) return rc;
  HIP_TRY(c, mplx::launch_cloud_fill((const int8_t *)c->map.p, D, c->mdim, kind, offs, 0, total, c->res, c->origin, (double *)b->raw.p,
                                     c->stream));
  return end_fill(b, total);
}

int mplx_body_shape(mplx_body *b, int64_t *n, int64_t *n_excluded, int32_t *cells_per_axis, double *cell_edge, double *origin,
                    int64_t *generation) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  mplx::BodyGrid G{};
  if (b->binned) {
    if (int rc = bind_device(c)) return rc;
    HIP_TRY(c, hipMemcpyAsync(&G, b->hdr.p, sizeof G, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  if (n) *n = b->filled ? b->n : 0;
  if (n_excluded) *n_excluded = b->binned ? b->n - G.n_incl : 0;
  for (int d = 0; d < 3; d++) {
    if (cells_per_axis) cells_per_axis[d] = b->binned ? G.dims[d] : 0;
    if (origin) origin[d] = G.origin[d];
  }
  if (cell_edge) *cell_edge = G.edge;
  if (generation) *generation = b->generation;
  return MPLX_OK;
}

int mplx_body_cells(mplx_body *b, int32_t *h_cell_of_point, int32_t *h_cell_start) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  if (int rc = ready(b, "mplx_body_cells")) return rc;
  if (int rc = bind_device(c)) return rc;
  mplx::BodyGrid G{};
  HIP_TRY(c, hipMemcpyAsync(&G, b->hdr.p, sizeof G, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (G.n_cells < 1 || G.n_cells > mplx::kBodyMaxCells) return fail(c, MPLX_ERR_HIP, "mplx_body_cells: the grid header is damaged");
  if (b->n > 0) HIP_TRY(c, stage_out(c, h_cell_of_point, b->cop.p, (size_t)b->n * 4));
  HIP_TRY(c, stage_out(c, h_cell_start, b->cells.p, ((size_t)G.n_cells + 1) * 4));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

int mplx_body_check_device(mplx_body *b, const mplx_succ_lists *L, int64_t n_nodes, const int32_t *d_parent_id,
                           const double *d_parent_state, int64_t parent_stride, int32_t n_samp, int64_t *d_hit, int64_t *d_n_blocked) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  const char *who = "mplx_body_check_device";
  if (!L || n_nodes < 0 || !d_parent_id || !d_parent_state) return fail(c, MPLX_ERR_ARG, "%s: NULL argument or n_nodes < 0", who);
  if (!L->count || !L->action || !L->cost) return fail(c, MPLX_ERR_ARG, "%s: the lists need count, action and cost", who);
  if (n_samp < 1) return fail(c, MPLX_ERR_ARG, "%s: n_samp must be >= 1", who);
  const int64_t S = list_stride(c, L);
  if (S < 1 || n_nodes > kMaxEntries / S) return fail(c, MPLX_ERR_ARG, "%s: node_stride < 1 or more than 2^31 - 2 list entries", who);
  if (parent_stride < n_nodes) return fail(c, MPLX_ERR_ARG, "%s: parent_stride < n_nodes", who);
  if (int rc = ready(b, who)) return rc;
  if (!c->has_params) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_params has not been called", who);
  if (!c->has_U) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_controls has not been called", who);
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // yaw pinning: the lists must be final
  if (n_nodes == 0) return MPLX_OK;
  mplx::BodyCheckArgs a{};
  a.shape = b->sh;
  a.cloud = cloud_of(b);
  a.count = L->count; a.action = L->action; a.cost = L->cost;
  a.n_rows = n_nodes; a.S = S;
  a.parent_id = d_parent_id; a.parent_state = d_parent_state; a.parent_stride = parent_stride;
  a.U = (const double *)c->U.p; a.nU = c->nU; a.udim = c->udim;
  a.dt = c->prm.dt;
  a.ds = c->prm.dt / (double)n_samp;
  a.n_samp = n_samp;
  // lanes over a row's entries: the smallest power of two >= S, at least 8, 64 at the most; the other lanes of the
  // wave split an entry's points (as reserve_api.cpp splits the reservations)
  int sp = 3;
  while ((1 << sp) < 64 && (1 << sp) < S) sp++;
  a.sp_log2 = sp;
  a.hit = (long long *)d_hit;
  a.n_blocked = (unsigned long long *)d_n_blocked;
  HIP_TRY(c, mplx::launch_body_check(c->dim, c->prm.control, a, c->stream));
  return MPLX_OK;
}

int mplx_body_check_poly_device(mplx_body *b, mplx_poly *p, const mplx_body_poly_in *in, const mplx_body_poly_out *d_out) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  if (int rc = check_poly_args(b, p, "mplx_body_check_poly_device", in, d_out)) return rc;
  if (p->n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  return poly_launch(b, p, in->step, d_out->hit, d_out->status, d_out->n_hit);
}

int mplx_body_check_poly(mplx_body *b, mplx_poly *p, const mplx_body_poly_in *in, const mplx_body_poly_out *h_out) {
  if (!b) return MPLX_ERR_ARG;
  mplx_ctx *c = b->c;
  if (int rc = check_poly_args(b, p, "mplx_body_check_poly", in, h_out)) return rc;
  if (p->n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  const size_t K = (size_t)p->n;
  StageLayout l;  // (only the carving)
  const size_t o_h = l.add(K * 8), o_n = l.add(8), o_s = l.add(K);
  if (int rc = ensure(c, b->rows, l.total)) return rc;
  char *base = (char *)b->rows.p;
  if (h_out->n_hit) HIP_TRY(c, stage_in(c, base + o_n, h_out->n_hit, 8));
  if (int rc = poly_launch(b, p, in->step, h_out->hit ? (int64_t *)(base + o_h) : nullptr, h_out->status ? (uint8_t *)(base + o_s) : nullptr,
                           h_out->n_hit ? (int64_t *)(base + o_n) : nullptr))
    return rc;
  HIP_TRY(c, stage_out(c, h_out->hit, base + o_h, K * 8));
  HIP_TRY(c, stage_out(c, h_out->status, base + o_s, K));
  HIP_TRY(c, stage_out(c, h_out->n_hit, base + o_n, 8));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

}  // extern "C"
