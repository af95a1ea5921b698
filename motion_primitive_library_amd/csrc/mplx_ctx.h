// mplx_ctx.h -- the context object behind the C ABI (include/mplx.h) and the small
// helpers every API translation unit uses.  Private to libmplx.so.
#ifndef MPLX_CTX_H
#define MPLX_CTX_H

#include "../../include/mplx.h"
#include "../../include/mplx_debug.h"
#include "../../include/mplx_open.h"  // mplx_open, mplx_table_frontier: what open_push() below takes
#include "../../include/mplx_traj.h"  // mplx_traj_set: what the traj_* helpers below take
#include "mplx_internal.h"
#include "mplx_stage.h"

#include <cstdarg>
#include <cstdio>
#include <exception>
#include <new>
#include <string>
#include <vector>

struct mplx_table;    // include/mplx_table.h
struct mplx_reserve;  // include/mplx_reserve.h

namespace mplx_detail {

struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
};

std::string &create_error();  // text of the last failed mplx_create (thread local)

}  // namespace mplx_detail

struct mplx_ctx {
  int dim = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::string err;

  // environment (device copies)
  mplx_detail::DevBuf map, pot, region_bits, region_bytes, U;
  bool has_map = false, has_pot = false, has_region = false, has_params = false, has_U = false;
  // mplx_set_goal: the goal the heur / flags rows of mplx_succ_lists refer to (PostFuse without its output pointers)
  bool has_goal = false;
  mplx::PostFuse goal_fuse{};
  int32_t goal_ctl[2] = {0, 0};  // control and goal_control of that goal (include/mplx_heur.h: the push with ROBUST)
  int32_t mdim[3] = {1, 1, 1};
  double origin[3] = {0, 0, 0};
  double res = 0;
  int64_t n_cells = 0;
  uint64_t map_upload_bytes = 0;  // host -> device bytes of mplx_set_map / _set_potential / _set_region / _edit_map so far
  mplx_params prm{};
  int32_t nU = 0, udim = 0;
  double u_absmax = 0;  // max |u| over the spatial control entries
  // per-axis factorisation of the control table (expand_grid_kernel.hip)
  mplx_detail::DevBuf uvals, uidx, blk, sat;
  bool sat_ok = false;   // summed-area table of blk is current
  mplx_detail::DevBuf post_keys;                 // node-identity table (post_api.cpp)
  mplx_detail::DevBuf post_ws;                   // workspace of the partitioned identity pass (identity_kernel.hip)
  mplx_detail::DevBuf ray_work;                  // candidate worklist of mplx_goal_sight_device (ray_api.cpp)
  mplx_detail::DevBuf heur_ws;                   // state rows and h of mplx_heur_eval (heur_api.cpp): its own block, not the arena
  mplx_detail::DevBuf traj_tab;                  // segment table of the trajectory calls (traj_api.cpp); grow-only
  mplx_detail::DevBuf conflict_ws;               // scratch of mplx_traj_conflicts (conflict_api.cpp); grow-only
  mplx_detail::DevBuf prep_lut, prep_a, prep_b;  // map preprocessing scratch (map_prep_api.cpp)
  bool blk_ok = false;   // blocked-bit map matches the current map + region
  uint64_t blk_epoch = 0;  // bumped wherever blk_ok is cleared or the bits are patched: what a goal field was built at (include/mplx_field.h)
  bool u_factored = false;
  bool u_wide = false;   // 17 .. 32 distinct values on some axis: only the lexicographic kernel (expand_lex_kernel.hip) takes the table
  bool u_lex = false;    // the table is the full Cartesian product of its per-axis values in lexicographic order
  int32_t u_nd[4] = {0, 0, 0, 0};  // distinct control values per axis; [3] = yaw rates
  // Diagnostic knobs, read from the environment once per context (mplx_create): ablations and forced code paths
  // for tests and profiling scripts; all off / automatic in production.
  struct Tuning {
    int grid_rmax = 0, grid_boxcap = 0, grid_blocks = 0;  // MPLX_GRID_RMAX / _BOXCAP / _BLOCKS (0 = automatic)
    int grid_waves_per_cu = 0;                            // MPLX_GRID_WAVES_PER_CU: occupancy cap (0 = automatic)
    int grid_gather = -1, grid_sat = -1;                  // MPLX_GRID_GATHER / MPLX_GRID_SAT: force 0 / 1 (-1 = automatic)
    bool grid_lex = true;                                 // MPLX_GRID_LEX=0: lexicographic tables run expand_grid_kernel like every other table
    bool grid_static = false;                             // MPLX_GRID_STATIC: static node striding instead of the work counters
    int grid_chunk = 0;                                   // MPLX_GRID_CHUNK: nodes per claim (0 = automatic)
    int grid_blocked = 0;                                 // MPLX_GRID_BLOCKED: contiguous shares per counter (A/B)
    int dbg = 0;                                         // MPLX_TILE_DBG ablation bits
    bool no_pair = false;                                // MPLX_GRID_PAIR=0: pre-screened yaw + potential launches stay with expand_grid_kernel
    int pair_rmax = 0, pair_wg_per_cu = 0;               // MPLX_PAIR_RMAX / MPLX_PAIR_WG_PER_CU: rows per pass / resident workgroups of expand_pair_kernel
    int zero_copy = 1;                                   // MPLX_ZERO_COPY=0: small batches through a device arena instead
    int arena_kb = 0;                                    // MPLX_ARENA_KB: largest batch served by the one-copy path
    bool no_sat = false, no_lex = false, no_line_pad = false;  // MPLX_GRID_NOSAT / MPLX_GRID_NOLEX / MPLX_NO_LINE_PAD
    int prescreen_min = 0;     // MPLX_GRID_PRESCREEN_MIN: smallest frontier that gets the lane-per-node pre-screen (0 = automatic, -1 = never)
    bool yaw_pin = true;       // MPLX_YAW_PIN=0: raw device trig decisions (to measure what the pinning is for)
    double yaw_margin = 0;     // MPLX_YAW_MARGIN: detection band (tests widen it to drive many nodes through the fix pass)
    int done_flag = 1;         // MPLX_DONE_FLAG=0: small synchronous launches end with hipStreamSynchronize (DoneSignal)
    int service = 1;           // MPLX_SERVICE=0: every small batch is its own launch (mplx_service)
    int service_idle_us = 500;    // MPLX_SERVICE_IDLE_US: the resident kernel leaves after this long without a request
    int service_max_nodes = 256;  // MPLX_SERVICE_MAX_NODES: larger batches are launches of their own
    int reserve_lanes = 0;        // MPLX_RESERVE_LANES: lanes of a wave over a row's entries in reserve_kernel.hip, a power of two (0 = automatic)
  } tune;
  int lists_route = MPLX_ROUTE_AUTO;
  int last_route = MPLX_ROUTE_AUTO;
  uint32_t last_zero_rows = 0;  // state rows the last lists launch did not store to (mplx_last_lists_zero_rows)
  bool last_grid_pair = false;  // ... or to expand_pair_kernel.hip
  bool last_grid_lex = false;  // the last factorised launch went to expand_lex_kernel.hip (mplx_debug_last_kernel)
  int n_cus = 256;

  // tables of the tiled kernel (sample times, loop counts, reciprocals)
  mplx_detail::DevBuf tables;
  bool tables_ok = false;
  double tab_dt = 0, tab_res = 0;
  double recips[3] = {0, 0, 0};
  // scratch for the dense -> lists route
  mplx_detail::DevBuf d_status, d_cost, d_hash, d_state, d_iters;
  // The one device block every host-pointer entry point stages its arrays in for the length of the call (StageLayout
  // below states the rules), and the pinned mirror of the small batches of mplx_expand_lists (lists_host.cpp).
  mplx_detail::DevBuf s_arena;
  void *h_arena = nullptr;
  size_t h_arena_cap = 0;
  // Completion of small synchronous launches through a word the kernel writes itself (DoneSignal, mplx_internal.h)
  uint64_t *done_host = nullptr;     // pinned
  mplx_detail::DevBuf done_count;    // 4 bytes, zero between launches
  uint64_t done_seq = 0;
  bool want_done = false;            // set by a caller that will wait for the launch on the spot (around lists_device)
  bool done_armed = false;           // ... and the launch that went in carries the signal
  int64_t done_waits = 0, done_timeouts = 0;
  // Resident form of the tiled kernel for the small synchronous batches of a search ("service", lists_host.cpp and
  // expand_tile_kernel.hip): requests go through a mailbox in pinned memory instead of launch + synchronise.
  struct Service {
    bool running = false;   // a resident kernel has been launched and has not been seen to leave
    bool disabled = false;  // it failed to answer once: never again in this context
    int streak = 0;         // eligible batches since the last other API call (the second one starts the service)
    hipStream_t stream = nullptr;
    mplx::SvcMailbox *mb = nullptr;  // pinned
    char *block = nullptr;           // pinned landing block: node rows, then the list rows, sized for `cap` nodes
    size_t block_cap = 0;
    mplx_detail::DevBuf dev;         // command word + one word per workgroup
    uint32_t seq = 0;
    int64_t cap = 0, S = 0;          // signature of the resident kernel: capacity in nodes, list stride,
    unsigned rows = 0;               // ... and which list rows it writes (bit 0 action, 1 cost, 2 hash, 3 iters, 4 state)
    int workgroups = 0;
    int64_t requests = 0, launches = 0, failures = 0;  // statistics (mplx_service)
  } svc;
  // pipelined copy back of the lists (lists_copy_api.cpp): packed chunks on the device, pinned landing buffers
  mplx_detail::DevBuf pk_dev[2], pk_offs;
  void *pk_pin[2] = {nullptr, nullptr};
  size_t pk_pin_cap = 0;
  hipEvent_t pk_ev[2] = {nullptr, nullptr};
  std::vector<int64_t> pk_hoffs;
  void *pk_hb = nullptr;  // pinned block of expand_lists_packed: nodes, counts, offsets
  size_t pk_hb_cap = 0;
  // yaw pinning (YawPin, mplx_internal.h): launches whose heading-limit decisions have not been checked against
  // the host libm yet; resolved by resolve_pending() at the next synchronising call
  struct YawPending {
    int kind = 0;  // 0: factorised lists kernel, 1: dense kernel
    mplx::GridArgs g{};
    mplx::ExpandArgs e{};
  };
  std::vector<YawPending> yaw_pending;
  int32_t *yaw_any_host = nullptr;  // pinned word: some launch since the last resolve flagged a node
  int32_t *id_ovf_host = nullptr;   // pinned word: a bucket of the claimed identity pass overflowed (post_api.cpp)
  bool sat_stale = false;           // the blocked bits were patched by mplx_edit_map: the summed-area table waits for a launch worth rebuilding it for
  int id_backoff = 0;               // calls left that skip the claimed identity form after an overflow (post_api.cpp)
  int last_identity_form = 0;       // 0 none / table in HBM, 1 claimed, 2 exact partition, 3 claimed then exact (overflow)
  mplx_detail::DevBuf yaw_ring, yaw_ids, yaw_tab;  // flagged nodes per pending launch; node list + trig table of a fix pass
  std::vector<double> h_U;          // host copy of the control table (the fix pass needs the yaw rates)
  double h_uyaw[16] = {0};          // ... and of its distinct yaw rates, in the factorisation's order
  int64_t yaw_flagged = 0, yaw_fix_passes = 0;  // statistics (mplx_yaw_pin_stats)
  mplx_detail::DevBuf live_list;          // pre-screen of yaw controls: surviving nodes (int32 each)
  mplx_detail::DevBuf live_ctr;           // ... and their number: two counters used alternately (live_parity), zero between launches
  int live_parity = 0;
  mplx_detail::DevBuf work_counter;       // dynamic node assignment of the factorised kernel (GridArgs::work)
  int work_parity = 0;                    // which of the two counter sets the next launch uses
  // workgroups of the factorised kernel resident per CU (grid_resident_blocks), cached per (control, potential, LDS)
  struct GridOcc { int control; bool pot; size_t lds; int nb; };
  mutable std::vector<GridOcc> grid_occ;
  // RCCL communicator of this context (comm_api.cpp); the library is loaded on first use
  void *comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  mplx_detail::DevBuf comm_meta;  // [world + 1][MPLX_COMM_META] int64: the meta record of every rank, then the own one
  std::vector<double> h_state;  // mplx_get_succ: the state rows of its one node
};

// include/mplx_field.h (field_api.cpp); open_api.cpp reads it for the push of an open set with a field
struct mplx_field {
  mplx_ctx *c = nullptr;
  mplx_detail::DevBuf dist, active, counter;
  mplx_detail::DevBuf bits;  // with a potential map installed: the field's own blocked bits (field_kernel.hip says why)
  std::vector<mplx_open *> users;  // the open sets it is in force in: told when it is destroyed (open_field_gone)
  int32_t F = 0;           // 0: empty
  int64_t n_cells = 0;     // ... of the map the field was built on
  uint64_t epoch = 0;      // mplx_ctx::blk_epoch at the build
  int64_t passes = 0;      // of the last build (diagnostic)
};

namespace mplx_detail {

inline int fail(mplx_ctx *c, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else create_error() = buf;
  return code;
}

#define HIP_TRY(c, expr)                                                                   \
  do {                                                                                     \
    hipError_t e__ = (expr);                                                               \
    if (e__ != hipSuccess)                                                                 \
      return mplx_detail::fail((c), MPLX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                  __FILE__, __LINE__);                                                     \
  } while (0)

// No exception may cross the C ABI (include/mplx.h: "never throws"): entry points that touch std containers wrap
// their bodies in these.
#define MPLX_GUARD_BEGIN try {
#define MPLX_GUARD_END(c)                                                                            \
  }                                                                                                  \
  catch (const std::bad_alloc &) { return mplx_detail::fail((c), MPLX_ERR_NOMEM, "out of host memory"); } \
  catch (const std::exception &e) { return mplx_detail::fail((c), MPLX_ERR_NOMEM, "unexpected exception: %s", e.what()); } \
  catch (...) { return mplx_detail::fail((c), MPLX_ERR_NOMEM, "unexpected exception"); }

int svc_stop(mplx_ctx *c);  // lists_host.cpp (the other declarations of that unit: below)

// Every entry point that touches the device comes through here first.  A resident service kernel reads the
// context's tables through the arguments it was launched with and writes into the context's landing block: it is
// asked to leave before anything else happens (only the small-batch path of mplx_expand_lists talks to it instead).
inline int bind_device(mplx_ctx *c) {
  HIP_TRY(c, hipSetDevice(c->device));
  c->svc.streak = 0;
  if (c->svc.running) return svc_stop(c);
  return MPLX_OK;
}

inline int ensure(mplx_ctx *c, DevBuf &b, size_t bytes) {
  if (bytes <= b.cap) return MPLX_OK;
  if (b.p) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  HIP_TRY(c, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return MPLX_OK;
}

inline void release(DevBuf &b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

// ---- Staging of host arrays on the device: rows carved out of mplx_ctx::s_arena for the length of one call.
//  1. A call lays out everything it stages and commits ONCE, before it enqueues its first copy: ensure() synchronises
//     and frees on growth, so a second growth would lose the copies already enqueued.
//  2. When a host-pointer entry point returns, no launch or copy that reads or writes the arena is outstanding (each
//     ends in a synchronise, in resolve_pending, or in the wait of its small-batch launch).
//  3. A call that enters another entry point while it holds arena rows has first copied everything it still needs to
//     the host: the inner call carves the same block.
//  4. Device-pointer entry points never touch the arena.  It only grows: the rounded rows of the largest call so far.
// A host twin declares its rows once in a StageRows (mplx_stage.h: offsets and sizes, no HIP) and the rules are kept by
// the two functions below:
//  1. stage_commit(c, &s): the only ensure() of the arena in a call, then every input copy, in declaration order.  A row
//     cannot be added afterwards with any effect: its device side is read through s.dev() only after the commit.
//  2. stage_fetch(c, &s): every output copy, in declaration order, and the synchronise the twin ends with.  A twin that
//     ends in a read-back of its own (seed_table: read_count; mplx_field_build: its passes) synchronises there instead.
//  3. is the caller's: after stage_fetch its landed rows are host memory (s.host()), so it may enter another entry point.
//  4. _device forms take no StageRows and no StageLayout: nothing in them can name the arena.
// The StageRows of a call lives on its stack; no object keeps a pointer into it or into the arena.
// Still on the raw layer (StageLayout + stage_in / stage_out), because their shape is not "copy in, launch, copy out,
// synchronise":
//   mplx_expand_lists, lists_host.cpp, lists_copy_api.cpp, expand_lists_packed -- zero-copy landing, the service kernel,
//     deferral through resolve_pending;
//   mplx_rollout (first site) -- reads the status row and synchronises first: where the other rows land depends on it;
//   mplx_table_path -- reads the length first, then only that many ids and actions;
//   mplx_heur_eval -- carves a block of its own (mplx_ctx::heur_ws), not the arena.
inline int stage_commit(mplx_ctx *c, StageLayout *l) {
  if (int rc = ensure(c, c->s_arena, l->total)) return rc;
  l->base = (char *)c->s_arena.p;
  return MPLX_OK;
}
// The copies, on the context's stream, for HIP_TRY at the call site.  In: one row / `rows` host rows of `width` bytes,
// `src_stride` bytes apart, to packed device rows.  Out, if the caller asked for the row (host != null): the reverse.
inline hipError_t stage_in(mplx_ctx *c, void *dev, const void *host, size_t bytes) {
  return hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, c->stream);
}
inline hipError_t stage_in_rows(mplx_ctx *c, void *dev, const void *host, size_t src_stride, size_t width, size_t rows) {
  return hipMemcpy2DAsync(dev, width, host, src_stride, width, rows, hipMemcpyHostToDevice, c->stream);
}
inline hipError_t stage_out(mplx_ctx *c, void *host, const void *dev, size_t bytes) {
  return host ? hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}
inline hipError_t stage_out_rows(mplx_ctx *c, void *host, size_t dst_stride, const void *dev, size_t width, size_t rows) {
  return host ? hipMemcpy2DAsync(host, dst_stride, dev, width, width, rows, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}

// The rows of a call (StageRows): carve them, then the input copies in declaration order ...
inline int stage_commit(mplx_ctx *c, StageRows *s) {
  if (s->overflow) return fail(c, MPLX_ERR_ARG, "more than %d staged rows in one call", StageRows::kMaxRows);
  if (s->land_total && !(s->landing = (char *)::operator new(s->land_total, std::nothrow))) return fail(c, MPLX_ERR_NOMEM, "out of host memory");
  if (int rc = stage_commit(c, &s->l)) return rc;
  for (int i = 0; i < s->n; i++) {
    const StageRows::Rec &r = s->rec[i];
    if (!r.src) continue;
    HIP_TRY(c, r.pitch ? stage_in_rows(c, s->l.base + r.at, r.src, r.pitch, r.width, r.rows) : stage_in(c, s->l.base + r.at, r.src, r.bytes));
  }
  return MPLX_OK;
}
// ... and after the launches the output copies in declaration order and the one synchronise of the call.
inline int stage_fetch(mplx_ctx *c, StageRows *s) {
  for (int i = 0; i < s->n; i++) {
    const StageRows::Rec &r = s->rec[i];
    if (r.land) HIP_TRY(c, stage_out(c, s->landing + r.land_at, r.from ? r.from : s->l.base + r.at, r.land));
    else if (r.dst) HIP_TRY(c, r.pitch ? stage_out_rows(c, r.dst, r.pitch, s->l.base + r.at, r.width, r.rows) : stage_out(c, r.dst, s->l.base + r.at, r.bytes));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MPLX_OK;
}

// The per-node lists of a host frontier, left packed in the context's pinned landing buffer (node k owns entries
// [offs[k], offs[k+1]) of every row): for callers inside the library that consume the lists at once (the host search,
// planner_capi.cpp) and would only copy them again.  Valid until the next call on the context.
struct PackedLists {
  int64_t total = 0;
  const int32_t *count = nullptr;   // [n_nodes]
  const int64_t *offs = nullptr;    // [n_nodes + 1]
  const double *cost = nullptr;     // [total]
  const uint64_t *hash = nullptr;   // [total]
  const int32_t *action = nullptr;  // [total]
  const double *state = nullptr;    // [4D+2][total]
  const double *heur = nullptr;     // [total] default heuristic of every successor (want_heur; needs mplx_set_goal)
};
int expand_lists_packed(mplx_ctx *c, const double *h_nodes, int64_t n_nodes, int64_t node_stride, bool want_state,
                        PackedLists *out, bool want_heur = false);  // want_state = false: out->state == nullptr, the kernel skips the states
// ---- what crosses the boundaries of the API translation units (every such function is declared here and only here)

constexpr size_t kLdsBudget = 160 * 1024;   // LDS of a CU: what the workgroups resident on it share
constexpr size_t kTcntOffset = 64 * 64 * 8; // mplx_ctx::tables: ttab [64][64] doubles, then tcnt [64] bytes, then 3 reciprocals

// entries reserved per node in the rows of `o` (mplx_succ_lists::node_stride, 0 = one per control)
inline int64_t list_stride(const mplx_ctx *c, const mplx_succ_lists *o) { return o->node_stride ? o->node_stride : c->nU; }

// Line padding (expand_grid_kernel.hip) pays where a launch is bound by its stores -- the large control tables (C4: 729,
// 17^3).  With short lists it only adds bytes: C5 (81 controls, 24 successors per live node) writes 23.1 MB padded and
// 18.8 MB unpadded in the same 46.5 us, C3 and C2 likewise (profiles/r06_line_pad_small_lists.txt).
inline int line_pad(const mplx_ctx *c, int64_t stride) {
  return (stride % 32 == 0 && !c->tune.no_line_pad && c->nU >= mplx::kLinePadMinControls) ? 1 : 0;
}

// derivative order of the control input: 1 VEL .. 4 SNP (the yaw bit is ignored)
inline int control_order(int control) {
  const int ctl = control & 0x0f;
  return ctl == MPLX_VEL ? 1 : ctl == MPLX_ACC ? 2 : ctl == MPLX_JRK ? 3 : 4;
}

// mplx_api.cpp: map, parameters and controls are set and fit each other
int ctx_ready(mplx_ctx *c);

// lists_route.cpp: the route dispatch behind mplx_expand_lists* (GRID / TILE / DENSE), its plans and argument blocks.
struct TilePlan {
  bool ok = false;
  int npb = 1, tile_pairs = 0, wl_cap = 0, n_max = 0, u_offset = 0, grid = 0;
};
TilePlan plan_tile(const mplx_ctx *c);
int ensure_tables(mplx_ctx *c);
int ensure_blocked_bits(mplx_ctx *c);  // the blocked-bit map of the current map + region + potential, built if not current
mplx::ExpandArgs expand_args(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride, const mplx_succ *o);
mplx::TileArgs tile_args(mplx_ctx *c, const TilePlan &tp, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                         const mplx_succ_lists *o);
int launch_grid(mplx_ctx *c, mplx::GridArgs *a);
int lists_device(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride, const mplx_succ_lists *o,
                 uint32_t *zero_rows = nullptr);

// yaw_pin.cpp: heading-limit decisions pinned to the host libm (YawPin, mplx_internal.h).  yaw_slot: the detection block
// of the next launch.  resolve_pending: synchronises the stream and, where a launch flagged decisions within rounding
// noise of their threshold, re-expands those nodes with the host libm's trig values.  Every synchronising entry point
// and every call that changes what a pending launch read goes through it.
int yaw_slot(mplx_ctx *c, mplx::YawPin *y);
int resolve_pending(mplx_ctx *c, bool stream_is_idle = false);

// lists_host.cpp: the host-pointer lists calls and the resident service kernel behind their small batches.
int svc_request(mplx_ctx *c, const double *h_nodes, int64_t n_nodes, int64_t node_stride, const mplx_succ_lists *h_out,
                bool *handled, mplx_succ_lists *view);
// after a small-batch launch through lists_device with want_done set: waits for it (kernel-written word, or the
// stream); *idle = everything enqueued on the context's stream so far is complete
int wait_small_launch(mplx_ctx *c);

// lists_copy_api.cpp: device lists -> host lists, only the used prefixes, pipelined through pinned memory
int copy_lists_to_host(mplx_ctx *c, const mplx_succ_lists &d, const mplx_succ_lists *h_out, int64_t n_nodes);
void release_copy_buffers(mplx_ctx *c);


// table_api.cpp: the table as its open set (open_api.cpp) sees it.  table_open_args: the table's context, MPLX_ERR_STATE
// (with `who` in the text) once the host has seen a status bit, else the table fields of `a`.  table_observe: after a
// wait for the stream, what the last finished call left (status bit, node count).
int table_open_args(mplx_table *t, const char *who, mplx_ctx **c, mplx::OpenArgs *a);
void table_observe(mplx_table *t);
// ... and as a rebase (replan_api.cpp) sees it: the same check, the table's arrays, its bound of n_nodes and the scratch
// of the rebase passes (scratch: allocated here on the first call, for the table's capacity; the device is bound.  Without
// it only the check, n_queries and n_bound)
// time_keys: null refuses a table with time keys (the untimed rebases); else it receives whether the table has them
int table_replan_args(mplx_table *t, const char *who, bool scratch, mplx_ctx **c, mplx::ReplanArgs *a, int32_t *time_keys = nullptr);
// reserve_api.cpp: a reservation table as the timed rebase (replan_api.cpp) sees it: its context (set whatever it
// answers), MPLX_ERR_STATE before a fill or before mplx_reserve_set_queries, else the table, query, control and scan
// fields of `a` (the lists stay empty)
int reserve_table_args(mplx_reserve *r, const char *who, mplx_ctx **c, mplx::ReserveArgs *a);
// ... and as the check of a solved set (reserve_poly_api.cpp) sees it: MPLX_ERR_STATE before a fill only; the table
// fields, Q (0 before mplx_reserve_set_queries) and, where Q >= 1, the query fields
int reserve_fill_args(mplx_reserve *r, const char *who, mplx_ctx **c, mplx::ReserveArgs *a);
// wait_api.cpp: the zero action of include/mplx_wait.h -- the smallest all-zero row of the control table -- or -1
int32_t zero_action(const mplx_ctx *c);
// ... and as the check of a reservation table (reserve_api.cpp) sees it: the same check, the per-node query column (null
// for one query), the number of queries and the node capacity
int table_reserve_args(mplx_table *t, const char *who, mplx_ctx **c, const int32_t **d_query, int32_t *n_queries, int64_t *cap);
// open_api.cpp: mplx_open_push_device; closed: without IS_OPEN (mplx_open_push_closed_device, replan_api.cpp)
int open_push(mplx_open *o, const char *who, const mplx_table_frontier *d_rows, int64_t n_max, double eps, int32_t sight, bool closed);
// open_api.cpp: the open set as the park veto of a reservation table (reserve_api.cpp) sees it: its context and table
// (set whatever it answers), MPLX_ERR_STATE for a table with a status bit, else the table fields and the flags of `a`
int open_park_args(mplx_open *o, const char *who, mplx_ctx **c, mplx_table **tab, mplx::OpenArgs *a);
// open_api.cpp: the field in force in `o` is being destroyed (field_api.cpp): every later push is MPLX_ERR_STATE until the
// open set is given another field, clear_field or new goals
void open_field_gone(mplx_open *o);

// traj_api.cpp: the checks of a trajectory set, the chain launch into the context's segment table, and the staging of a
// host set (rows declared by traj_set_rows; after the commit traj_set_view gives the device set), for conflict_api.cpp.
int traj_check_set(mplx_ctx *c, const char *who, const mplx_traj_set *s, const void *out);
int traj_build_table(mplx_ctx *c, const mplx_traj_set *s, mplx::TrajArgs *out);
struct TrajSetRows { StageRows::Row starts, actions; };
TrajSetRows traj_set_rows(const mplx_ctx *c, const mplx_traj_set *s, StageRows *st);
mplx_traj_set traj_set_view(const mplx_traj_set *s, const StageRows &st, const TrajSetRows &r);

// mplx_api.cpp: a goal as the kernels take it (mplx_set_goal's checks and hash), for the goals of an open set.
int goal_fuse_of(mplx_ctx *c, const char *who, const mplx_goal_spec *g, mplx::PostFuse *out);
// ray_api.cpp: mplx_goal_sight_device with the goal per list entry -- entry i aims at d_goals[d_row_query[i]].goal; tol:
// the largest tol_pos among the goals.  Read for candidates only (entries within their count whose flags have bit 0).
int goal_sight_rows(mplx_ctx *c, const mplx_succ_lists *d_lists, int64_t n_nodes, const int32_t *d_row_query,
                    const mplx::PostFuse *d_goals, double tol, uint8_t *d_flags);

}  // namespace mplx_detail
#endif
