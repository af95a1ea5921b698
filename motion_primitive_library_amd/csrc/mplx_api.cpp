// mplx_api.cpp -- the context behind the C ABI of libmplx.so (declared in include/mplx.h): create / destroy, the
// setters, the dense mplx_expand*, the device utilities and the diagnostics.  The lists calls live beside it:
// lists_route.cpp (mplx_expand_lists_device*, the GRID / TILE / DENSE dispatch), yaw_pin.cpp (heading-limit decisions
// pinned to the host libm), lists_host.cpp (mplx_expand_lists, mplx_get_succ, the resident service kernel).
//
// Owns the per-context HIP state: one stream, the HBM-resident copies of the
// map / potential / search-region / control table, staging buffers for the
// host-pointer convenience calls, and a pair of events used as a stopwatch.
// There is deliberately no CPU implementation behind this ABI: every compute
// entry either runs the gfx950 kernels or returns an error.
#include "mplx_ctx.h"
#include "host_planner.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace mplx_detail;

namespace mplx_detail {
std::string &create_error() {
  thread_local std::string e;
  return e;
}

int ctx_ready(mplx_ctx *c) {
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "mplx_set_map has not been called");
  if (!c->has_params) return fail(c, MPLX_ERR_STATE, "mplx_set_params has not been called");
  if (!c->has_U) return fail(c, MPLX_ERR_STATE, "mplx_set_controls has not been called");
  const int need = c->dim + ((c->prm.control & 0x10) ? 1 : 0);
  if (c->udim < need)
    return fail(c, MPLX_ERR_STATE, "controls have %d entries per row, control flag 0x%x needs %d",
                c->udim, c->prm.control, need);
  return MPLX_OK;
}
}  // namespace mplx_detail

namespace {

bool control_ok(int32_t control) {
  switch (control) {
    case MPLX_VEL: case MPLX_ACC: case MPLX_JRK: case MPLX_SNP:
    case MPLX_VELxYAW: case MPLX_ACCxYAW: case MPLX_JRKxYAW: case MPLX_SNPxYAW:
      return true;
    default:
      return false;
  }
}

}  // namespace

int mplx_detail::goal_fuse_of(mplx_ctx *c, const char *who, const mplx_goal_spec *g, mplx::PostFuse *out) {
  mplx::PostFuse f{};
  if (!g->goal) return fail(c, MPLX_ERR_ARG, "%s: goal waypoint is NULL", who);
  if (!control_ok(g->control) || (g->goal_control && !control_ok(g->goal_control)))
    return fail(c, MPLX_ERR_ARG, "%s: unknown control flag", who);
  const int F = 4 * c->dim + 2;
  for (int i = 0; i < F; i++) f.goal[i] = g->goal[i];
  // env_base.h:47 compares the goal with a state by hash, each side hashed with its own flags (waypoint.h:93-125)
  f.goal_hash = mplx::host::lattice_hash(c->dim, g->goal_control ? g->goal_control : g->control, g->goal);
  f.w = g->w; f.v_max = g->v_max;
  f.tol_pos = g->tol_pos; f.tol_vel = g->tol_vel; f.tol_acc = g->tol_acc; f.tol_yaw = g->tol_yaw;
  *out = f;
  return MPLX_OK;
}

extern "C" {

int mplx_abi_version(void) { return MPLX_ABI_VERSION; }

const char *mplx_last_error(const mplx_ctx *ctx) {
  return ctx ? ctx->err.c_str() : create_error().c_str();
}

int mplx_create(int dim, int device, mplx_ctx **out) {
  if (!out) return fail(nullptr, MPLX_ERR_ARG, "mplx_create: out is NULL");
  *out = nullptr;
  if (dim != 2 && dim != 3) return fail(nullptr, MPLX_ERR_ARG, "mplx_create: dim must be 2 or 3, got %d", dim);
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, MPLX_ERR_NO_DEVICE,
                "mplx_create: no HIP device available (%s); this engine has no CPU fallback",
                e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
  if (device < 0 || device >= count)
    return fail(nullptr, MPLX_ERR_ARG, "mplx_create: device %d out of range [0,%d)", device, count);
  mplx_ctx *c = new (std::nothrow) mplx_ctx();
  if (!c) return fail(nullptr, MPLX_ERR_ARG, "mplx_create: out of host memory");
  c->dim = dim;
  c->device = device;
  e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&c->ev0);
  if (e == hipSuccess) e = hipEventCreate(&c->ev1);
  if (e != hipSuccess) {
    fail(nullptr, MPLX_ERR_HIP, "mplx_create: HIP set-up failed: %s", hipGetErrorString(e));
    mplx_destroy(c);
    return MPLX_ERR_HIP;
  }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      c->n_cus = prop.multiProcessorCount;
  }
  {
    auto env_int = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : 0; };
    c->tune.grid_rmax = env_int("MPLX_GRID_RMAX");
    c->tune.grid_boxcap = env_int("MPLX_GRID_BOXCAP");
    c->tune.grid_blocks = env_int("MPLX_GRID_BLOCKS");
    c->tune.grid_waves_per_cu = env_int("MPLX_GRID_WAVES_PER_CU");
    c->tune.grid_static = getenv("MPLX_GRID_STATIC") != nullptr;
    if (getenv("MPLX_GRID_LEX")) c->tune.grid_lex = env_int("MPLX_GRID_LEX") != 0;
    c->tune.grid_chunk = env_int("MPLX_GRID_CHUNK");
    c->tune.grid_blocked = env_int("MPLX_GRID_BLOCKED");
    c->tune.grid_gather = getenv("MPLX_GRID_GATHER") ? env_int("MPLX_GRID_GATHER") : -1;
    c->tune.grid_sat = getenv("MPLX_GRID_SAT") ? env_int("MPLX_GRID_SAT") : -1;
    c->tune.dbg = env_int("MPLX_TILE_DBG");
    c->tune.no_pair = getenv("MPLX_GRID_PAIR") && env_int("MPLX_GRID_PAIR") == 0;
    c->tune.pair_rmax = env_int("MPLX_PAIR_RMAX");
    c->tune.pair_wg_per_cu = env_int("MPLX_PAIR_WG_PER_CU");
    c->tune.arena_kb = env_int("MPLX_ARENA_KB");
    c->tune.zero_copy = getenv("MPLX_ZERO_COPY") ? env_int("MPLX_ZERO_COPY") : 1;
    c->tune.no_sat = getenv("MPLX_GRID_NOSAT") != nullptr;
    c->tune.no_lex = getenv("MPLX_GRID_NOLEX") != nullptr;
    c->tune.no_line_pad = getenv("MPLX_NO_LINE_PAD") != nullptr;
    c->tune.prescreen_min = env_int("MPLX_GRID_PRESCREEN_MIN");
    c->tune.yaw_pin = !(getenv("MPLX_YAW_PIN") && atoi(getenv("MPLX_YAW_PIN")) == 0);
    c->tune.yaw_margin = getenv("MPLX_YAW_MARGIN") ? atof(getenv("MPLX_YAW_MARGIN")) : 0.0;
    if (getenv("MPLX_SERVICE")) c->tune.service = env_int("MPLX_SERVICE");
    if (getenv("MPLX_DONE_FLAG")) c->tune.done_flag = env_int("MPLX_DONE_FLAG");
    if (env_int("MPLX_SERVICE_IDLE_US") > 0) c->tune.service_idle_us = env_int("MPLX_SERVICE_IDLE_US");
    if (env_int("MPLX_SERVICE_MAX_NODES") > 0) c->tune.service_max_nodes = env_int("MPLX_SERVICE_MAX_NODES");
    if (env_int("MPLX_RESERVE_LANES") > 0) c->tune.reserve_lanes = env_int("MPLX_RESERVE_LANES");
  }
  if (c->tune.done_flag) {
    e = hipHostMalloc((void **)&c->done_host, 64, hipHostMallocCoherent);
    if (e == hipSuccess) { *c->done_host = 0; e = hipMalloc(&c->done_count.p, 64); }
    if (e == hipSuccess) { c->done_count.cap = 64; e = hipMemset(c->done_count.p, 0, 64); }
    if (e != hipSuccess) {
      fail(nullptr, MPLX_ERR_HIP, "mplx_create: HIP set-up of the completion word failed: %s", hipGetErrorString(e));
      mplx_destroy(c);
      return MPLX_ERR_HIP;
    }
  }
  if (c->tune.service) {
    // what the first resident kernel needs, now rather than inside the first search (stream, mailbox, command words and
    // a landing block for small control tables: ~1 ms of runtime calls otherwise paid by the first plan())
    mplx_ctx::Service &sv = c->svc;
    e = hipStreamCreateWithFlags(&sv.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void **)&sv.mb, sizeof(mplx::SvcMailbox), hipHostMallocCoherent);
    if (e == hipSuccess) {
      std::memset(sv.mb, 0, sizeof(mplx::SvcMailbox));
      e = hipHostMalloc((void **)&sv.block, (size_t)1 << 20, hipHostMallocCoherent);
    }
    if (e == hipSuccess) {
      sv.block_cap = (size_t)1 << 20;
      e = hipMalloc(&sv.dev.p, 1025 * 8);
    }
    if (e == hipSuccess) sv.dev.cap = 1025 * 8;
    if (e != hipSuccess) {
      fail(nullptr, MPLX_ERR_HIP, "mplx_create: HIP set-up of the service failed: %s", hipGetErrorString(e));
      mplx_destroy(c);
      return MPLX_ERR_HIP;
    }
  }
  *out = c;
  return MPLX_OK;
}

void mplx_destroy(mplx_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)mplx_detail::svc_stop(c);
  if (c->svc.stream) (void)hipStreamDestroy(c->svc.stream);
  if (c->svc.mb) (void)hipHostFree(c->svc.mb);
  if (c->svc.block) (void)hipHostFree(c->svc.block);
  release(c->svc.dev);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->done_host) (void)hipHostFree(c->done_host);
  release(c->done_count);
  for (DevBuf *b : {&c->map, &c->pot, &c->region_bits, &c->region_bytes, &c->U, &c->tables,
                    &c->d_status, &c->d_cost, &c->d_hash, &c->d_state, &c->d_iters, &c->uvals, &c->uidx, &c->blk, &c->sat, &c->prep_lut, &c->prep_a, &c->prep_b, &c->post_keys, &c->post_ws, &c->ray_work, &c->heur_ws, &c->traj_tab, &c->conflict_ws, &c->live_list, &c->live_ctr})
    release(*b);
  (void)mplx_comm_destroy(c);
  release(c->comm_meta);
  c->yaw_pending.clear();
  for (DevBuf *b : {&c->yaw_ring, &c->yaw_ids, &c->yaw_tab, &c->work_counter}) release(*b);
  if (c->yaw_any_host) (void)hipHostFree(c->yaw_any_host);
  if (c->id_ovf_host) (void)hipHostFree(c->id_ovf_host);
  mplx_detail::release_copy_buffers(c);
  release(c->s_arena);
  if (c->h_arena) (void)hipHostFree(c->h_arena);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int mplx_set_map(mplx_ctx *c, const int8_t *cells, const int32_t *dim, const double *origin, double res) {
  if (!c) return MPLX_ERR_ARG;
  if (!cells || !dim || !origin) return fail(c, MPLX_ERR_ARG, "mplx_set_map: NULL argument");
  if (!(res > 0)) return fail(c, MPLX_ERR_ARG, "mplx_set_map: resolution must be > 0");
  int64_t n = 1;
  for (int i = 0; i < c->dim; i++) {
    if (dim[i] <= 0) return fail(c, MPLX_ERR_ARG, "mplx_set_map: dim[%d] = %d", i, dim[i]);
    n *= dim[i];
  }
  if (n > 0x7fffffffLL)
    return fail(c, MPLX_ERR_ARG, "mplx_set_map: %lld cells exceed the reference's int cell index",
                (long long)n);
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // a pending launch read the old map
  {  // a different grid (size, shape, origin or resolution) invalidates potential and region
    bool same = n == c->n_cells && res == c->res;
    for (int i = 0; i < c->dim; i++) same = same && dim[i] == c->mdim[i] && origin[i] == c->origin[i];
    if (!same) {
      c->has_pot = false;
      c->has_region = false;
    }
  }
  if (int rc = ensure(c, c->map, (size_t)n)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->map.p, cells, (size_t)n, hipMemcpyHostToDevice, c->stream));
  c->map_upload_bytes += (uint64_t)n;
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // caller may free `cells` on return
  for (int i = 0; i < 3; i++) {
    c->mdim[i] = i < c->dim ? dim[i] : 1;
    c->origin[i] = i < c->dim ? origin[i] : 0.0;
  }
  c->res = res;
  c->n_cells = n;
  c->has_map = true;
  c->blk_ok = false;
  c->blk_epoch++;
  return MPLX_OK;
}

int mplx_set_potential(mplx_ctx *c, const int8_t *cells) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = resolve_pending(c)) return rc;
  if (!cells) {
    c->svc.streak = 0;
    if (int rc = mplx_detail::svc_stop(c)) return rc;  // (no resident kernel serves a potential map today: kept in step with mplx_set_region)
    c->blk_ok = c->blk_ok && !c->has_pot;
    c->blk_epoch++;
    c->has_pot = false;
    return MPLX_OK;
  }
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "mplx_set_potential: set the map first");
  if (int rc = bind_device(c)) return rc;
  if (int rc = ensure(c, c->pot, (size_t)c->n_cells)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->pot.p, cells, (size_t)c->n_cells, hipMemcpyHostToDevice, c->stream));
  c->map_upload_bytes += (uint64_t)c->n_cells;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->has_pot = true;
  c->blk_ok = false;
  c->blk_epoch++;
  return MPLX_OK;
}

int mplx_set_region(mplx_ctx *c, const uint8_t *cells) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = resolve_pending(c)) return rc;
  if (!cells) {
    c->svc.streak = 0;
    if (int rc = mplx_detail::svc_stop(c)) return rc;  // a resident kernel carries the region in its arguments
    c->blk_ok = c->blk_ok && !c->has_region;
    c->blk_epoch++;
    c->has_region = false;
    return MPLX_OK;
  }
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "mplx_set_region: set the map first");
  if (int rc = bind_device(c)) return rc;
  const size_t words = (size_t)((c->n_cells + 31) >> 5);
  if (int rc = ensure(c, c->region_bytes, (size_t)c->n_cells)) return rc;
  if (int rc = ensure(c, c->region_bits, words * 4)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->region_bytes.p, cells, (size_t)c->n_cells, hipMemcpyHostToDevice, c->stream));
  c->map_upload_bytes += (uint64_t)c->n_cells;
  HIP_TRY(c, mplx::launch_pack_region((const uint8_t *)c->region_bytes.p, (uint32_t *)c->region_bits.p,
                                      c->n_cells, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->has_region = true;
  c->blk_ok = false;
  c->blk_epoch++;
  return MPLX_OK;
}

int mplx_set_params(mplx_ctx *c, const mplx_params *p) {
  if (!c) return MPLX_ERR_ARG;
  if (!p) return fail(c, MPLX_ERR_ARG, "mplx_set_params: NULL");
  if (!control_ok(p->control)) return fail(c, MPLX_ERR_ARG, "mplx_set_params: unknown control flag 0x%x", p->control);
  if (!(p->dt > 0)) return fail(c, MPLX_ERR_ARG, "mplx_set_params: dt must be > 0");
  if (int rc = resolve_pending(c)) return rc;
  if (int rc = mplx_detail::svc_stop(c)) return rc;  // a resident kernel carries the old parameters in its arguments
  c->prm = *p;
  c->has_params = true;
  return MPLX_OK;
}

int mplx_set_goal(mplx_ctx *c, const mplx_goal_spec *g) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = resolve_pending(c)) return rc;
  mplx::PostFuse f{};
  bool has = false;
  if (g) {
    if (int rc = mplx_detail::goal_fuse_of(c, "mplx_set_goal", g, &f)) return rc;
    has = true;
  }
  if (has != c->has_goal || std::memcmp(&f, &c->goal_fuse, sizeof(f)) != 0) {
    if (int rc = mplx_detail::svc_stop(c)) return rc;  // a resident kernel carries the old goal in its arguments
    c->goal_fuse = f;
    c->has_goal = has;
  }
  c->goal_ctl[0] = g ? g->control : 0;
  c->goal_ctl[1] = g ? g->goal_control : 0;
  return MPLX_OK;
}

int mplx_set_controls(mplx_ctx *c, const double *U, int32_t nU, int32_t udim) {
  if (!c) return MPLX_ERR_ARG;
  if (!U || nU <= 0 || udim < c->dim || udim > c->dim + 1)
    return fail(c, MPLX_ERR_ARG, "mplx_set_controls: need U != NULL, nU > 0, udim in {%d,%d}", c->dim, c->dim + 1);
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t bytes = (size_t)nU * udim * sizeof(double);
  if (int rc = ensure(c, c->U, bytes)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->U.p, U, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->nU = nU;
  c->udim = udim;
  c->h_U.assign(U, U + (size_t)nU * udim);
  c->u_absmax = 0;
  for (int32_t i = 0; i < nU; i++)
    for (int k = 0; k < c->dim; k++) {
      const double a = std::fabs(U[(size_t)i * udim + k]);
      if (a > c->u_absmax) c->u_absmax = a;
    }
  // distinct values per spatial axis (compared bit-for-bit so that signed zeros stay apart): up to 16 per axis for the
  // factorised kernels at large, up to 32 for the lexicographic one (`wide`: expand_lex_kernel.hip alone takes it)
  c->u_factored = true;
  c->u_wide = false;
  double vals32[4][32] = {};
  std::vector<uint32_t> packed((size_t)nU, 0u);
  c->u_nd[3] = 0;
  for (int k = 0; k < udim && c->u_factored; k++) {
    const int slot = k < c->dim ? k : 3;  // the yaw rate (column dim of a yaw control table) is the fourth factor
    int n = 0;
    for (int32_t i = 0; i < nU; i++) {
      const double x = U[(size_t)i * udim + k];
      int j = 0;
      for (; j < n; j++)
        if (std::memcmp(&vals32[slot][j], &x, sizeof x) == 0) break;
      if (j == n) {
        if (n == 32) { c->u_factored = false; break; }
        vals32[slot][n++] = x;
      }
      packed[(size_t)i] |= (uint32_t)j << (8 * slot);
    }
    c->u_nd[slot] = n;
    if (n > 16) c->u_wide = true;
  }
  double vals[4][16] = {};
  for (int a4 = 0; a4 < 4; a4++) std::memcpy(vals[a4], vals32[a4], sizeof vals[a4]);
  c->u_lex = false;
  if (c->u_factored) {
    for (int k = c->dim; k < 3; k++) c->u_nd[k] = 0;
    // nested-loop tables (first axis slowest, yaw rate fastest): control i <-> the i-th index combination
    int64_t prod = 1;
    for (int k = 0; k < c->dim; k++) prod *= c->u_nd[k];
    const int ny = udim > c->dim ? c->u_nd[3] : 1;
    prod *= ny;
    if (prod == nU) {
      c->u_lex = true;
      for (int32_t i = 0; i < nU && c->u_lex; i++) {
        int32_t r = i;
        uint32_t want = 0;
        if (udim > c->dim) { want |= (uint32_t)(r % ny) << 24; r /= ny; }
        for (int k = c->dim - 1; k >= 0; k--) { want |= (uint32_t)(r % c->u_nd[k]) << (8 * k); r /= c->u_nd[k]; }
        c->u_lex = want == packed[(size_t)i];
      }
    }
    // a wide table is only of use to the lexicographic kernel: no yaw column, nested-loop order
    if (c->u_wide && (!c->u_lex || udim != c->dim)) c->u_factored = false;
  }
  if (c->u_factored) {
    std::memcpy(c->h_uyaw, vals[3], sizeof c->h_uyaw);
    if (int rc = ensure(c, c->uvals, sizeof vals + sizeof vals32)) return rc;  // [4][16], then [4][32]
    if (int rc = ensure(c, c->uidx, (size_t)nU * 4)) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->uvals.p, vals, sizeof vals, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync((char *)c->uvals.p + sizeof vals, vals32, sizeof vals32, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->uidx.p, packed.data(), (size_t)nU * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->has_U = true;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

int mplx_expand_device(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                       const mplx_succ *d_out) {
  if (!c) return MPLX_ERR_ARG;
  if (!d_out || n_nodes < 0 || node_stride < n_nodes || (!d_nodes && n_nodes > 0))
    return fail(c, MPLX_ERR_ARG, "mplx_expand_device: bad arguments");
  if (int rc = ctx_ready(c)) return rc;
  if (n_nodes == 0) return MPLX_OK;
  const int64_t n_slots = n_nodes * c->nU;
  if (d_out->state && d_out->state_stride < n_slots)
    return fail(c, MPLX_ERR_ARG, "mplx_expand_device: state_stride %lld < n_slots %lld",
                (long long)d_out->state_stride, (long long)n_slots);
  if (int rc = bind_device(c)) return rc;
  mplx::ExpandArgs a = expand_args(c, d_nodes, n_nodes, node_stride, d_out);
  a.stream_out = 1;
  if (int rc = yaw_slot(c, &a.yaw)) return rc;
  HIP_TRY(c, mplx::launch_expand(c->dim, c->prm.control, a, c->stream));
  if (a.yaw.amb) {
    mplx_ctx::YawPending p;
    p.kind = 1;
    p.e = a;
    c->yaw_pending.push_back(p);
  }
  return MPLX_OK;
}

int mplx_expand(mplx_ctx *c, const double *h_nodes, int64_t n_nodes, int64_t node_stride,
                const mplx_succ *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (!h_out || n_nodes < 0 || node_stride < n_nodes || (!h_nodes && n_nodes > 0))
    return fail(c, MPLX_ERR_ARG, "mplx_expand: bad arguments");
  if (int rc = ctx_ready(c)) return rc;
  if (n_nodes == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  const int F = 4 * c->dim + 2;
  const int64_t n_slots = n_nodes * c->nU;
  if (h_out->state && h_out->state_stride < n_slots)
    return fail(c, MPLX_ERR_ARG, "mplx_expand: state_stride < n_slots");
  // one arena block: the frontier packed to stride n_nodes, then the rows that were asked for
  const size_t slots = (size_t)n_slots;
  StageLayout l;
  const size_t o_nodes = l.add((size_t)F * n_nodes * 8), o_status = l.add(h_out->status ? slots : 0),
               o_cost = l.add(h_out->cost ? slots * 8 : 0), o_hash = l.add(h_out->hash ? slots * 8 : 0),
               o_iters = l.add(h_out->iters ? slots * 4 : 0), o_state = l.add(h_out->state ? F * slots * 8 : 0);
  if (int rc = stage_commit(c, &l)) return rc;
  HIP_TRY(c, stage_in_rows(c, l.base + o_nodes, h_nodes, (size_t)node_stride * 8, (size_t)n_nodes * 8, F));
  mplx_succ d{};
  if (h_out->status) d.status = (uint8_t *)(l.base + o_status);
  if (h_out->cost) d.cost = (double *)(l.base + o_cost);
  if (h_out->hash) d.hash = (uint64_t *)(l.base + o_hash);
  if (h_out->iters) d.iters = (int32_t *)(l.base + o_iters);
  if (h_out->state) { d.state = (double *)(l.base + o_state); d.state_stride = n_slots; }
  mplx::ExpandArgs a = expand_args(c, (const double *)(l.base + o_nodes), n_nodes, n_nodes, &d);
  a.stream_out = 1;
  if (int rc = yaw_slot(c, &a.yaw)) return rc;
  HIP_TRY(c, mplx::launch_expand(c->dim, c->prm.control, a, c->stream));
  if (a.yaw.amb) {
    mplx_ctx::YawPending p;
    p.kind = 1;
    p.e = a;
    c->yaw_pending.push_back(p);
    if (int rc = mplx_detail::resolve_pending(c)) return rc;
  }
  HIP_TRY(c, stage_out(c, h_out->status, d.status, slots));
  HIP_TRY(c, stage_out(c, h_out->cost, d.cost, slots * 8));
  HIP_TRY(c, stage_out(c, h_out->hash, d.hash, slots * 8));
  HIP_TRY(c, stage_out(c, h_out->iters, d.iters, slots * 4));
  HIP_TRY(c, stage_out_rows(c, h_out->state, (size_t)h_out->state_stride * 8, d.state, slots * 8, F));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

int mplx_device_alloc(mplx_ctx *c, size_t bytes, void **dptr) {
  if (!c) return MPLX_ERR_ARG;
  if (!dptr) return fail(c, MPLX_ERR_ARG, "mplx_device_alloc: NULL");
  *dptr = nullptr;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, hipMalloc(dptr, bytes ? bytes : 1));
  return MPLX_OK;
}

int mplx_device_free(mplx_ctx *c, void *dptr) {
  if (!c) return MPLX_ERR_ARG;
  if (!dptr) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipFree(dptr));
  return MPLX_OK;
}

int mplx_memcpy_h2d(mplx_ctx *c, void *dst, const void *src, size_t bytes) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = bind_device(c)) return rc;
  // the write may land in a frontier a pending launch read: its yaw fix pass re-reads the nodes, so it runs first
  if (int rc = resolve_pending(c)) return rc;
  HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

int mplx_memcpy_d2h(mplx_ctx *c, void *dst, const void *src, size_t bytes) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

int mplx_memset(mplx_ctx *c, void *dst, int value, size_t bytes) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // as mplx_memcpy_h2d
  HIP_TRY(c, hipMemsetAsync(dst, value, bytes, c->stream));
  return MPLX_OK;
}

int mplx_synchronize(mplx_ctx *c) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return resolve_pending(c);
}

int mplx_timer_begin(mplx_ctx *c) {
  if (!c) return MPLX_ERR_ARG;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  return MPLX_OK;
}

int mplx_timer_end(mplx_ctx *c, float *ms) {
  if (!c) return MPLX_ERR_ARG;
  if (!ms) return fail(c, MPLX_ERR_ARG, "mplx_timer_end: NULL");
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  HIP_TRY(c, hipEventSynchronize(c->ev1));
  HIP_TRY(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
  return resolve_pending(c);  // (after the measurement: a fix pass of the yaw pinning is not part of the timed launches)
}

int mplx_selftest_math(mplx_ctx *c, int op, const double *a, const double *b, double *out, int64_t n) {
  if (!c) return MPLX_ERR_ARG;
  if (!a || !out || n < 0 || (op == 0 && !b) || op < 0 || op > 5)
    return fail(c, MPLX_ERR_ARG, "mplx_selftest_math: bad arguments");
  if (n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  void *da = nullptr, *db = nullptr, *dout = nullptr;
  const size_t bytes = (size_t)n * sizeof(double);
  HIP_TRY(c, hipMalloc(&da, bytes));
  HIP_TRY(c, hipMalloc(&db, bytes));
  HIP_TRY(c, hipMalloc(&dout, bytes));
  HIP_TRY(c, hipMemcpyAsync(da, a, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(db, b ? b : a, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, mplx::launch_math_probe(op, (const double *)da, (const double *)db, (double *)dout, n, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return MPLX_OK;
}

int mplx_set_lists_route(mplx_ctx *c, int route) {
  if (!c) return MPLX_ERR_ARG;
  if (route < MPLX_ROUTE_AUTO || route > MPLX_ROUTE_GRID) return fail(c, MPLX_ERR_ARG, "mplx_set_lists_route: unknown route %d", route);
  c->lists_route = route;
  c->svc.streak = 0;
  return MPLX_OK;
}

int mplx_last_lists_route(const mplx_ctx *c) { return c ? c->last_route : MPLX_ERR_ARG; }
int mplx_last_lists_zero_rows(const mplx_ctx *c) { return c ? (int)c->last_zero_rows : MPLX_ERR_ARG; }
int mplx_last_grid_kernel(const mplx_ctx *c) {
  if (!c) return MPLX_ERR_ARG;
  if (c->last_route != MPLX_ROUTE_GRID) return MPLX_KERNEL_NONE;
  return c->last_grid_pair ? MPLX_KERNEL_PAIR : (c->last_grid_lex ? MPLX_KERNEL_LEX : MPLX_KERNEL_GRID);
}

int mplx_last_identity_form(const mplx_ctx *c) { return c ? c->last_identity_form : MPLX_ERR_ARG; }

int mplx_yaw_pin_stats(const mplx_ctx *c, int64_t *flagged_nodes, int64_t *fix_passes) {
  if (!c) return MPLX_ERR_ARG;
  if (flagged_nodes) *flagged_nodes = c->yaw_flagged;
  if (fix_passes) *fix_passes = c->yaw_fix_passes;
  return MPLX_OK;
}

int mplx_device_info(mplx_ctx *c, char *name, size_t cap, int32_t *compute_units) {
  if (!c) return MPLX_ERR_ARG;
  hipDeviceProp_t prop;
  HIP_TRY(c, hipGetDeviceProperties(&prop, c->device));
  if (name && cap) snprintf(name, cap, "%s (%s)", prop.name, prop.gcnArchName);
  if (compute_units) *compute_units = prop.multiProcessorCount;
  return MPLX_OK;
}

}  // extern "C"
