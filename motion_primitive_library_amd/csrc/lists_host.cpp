// lists_host.cpp -- the lists calls that take and return HOST pointers (mplx_expand_lists, mplx_get_succ) and what
// serves their small batches: one pinned block per call that the kernel reads and writes itself, and, for the batches
// of a search, the resident form of the tiled kernel (the "service": expand_tile_kernel.hip, SERVICE MODE).
#include "mplx_ctx.h"

#include <atomic>
#include <chrono>
#include <cstring>

using namespace mplx_detail;

namespace {

double mono_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// ---- the service: small synchronous batches through a resident kernel (expand_tile_kernel.hip, SERVICE MODE)
struct ArenaLayout {  // one block: node rows, counts, then the list rows that were asked for, all sized for n_alloc nodes
  size_t o_count = 0, o_action = 0, o_cost = 0, o_hash = 0, o_iters = 0, o_heur = 0, o_flags = 0, o_state = 0, total = 0;
  int64_t n_alloc = 0, n_slots = 0;
};
enum : unsigned { kRowAction = 1, kRowCost = 2, kRowHash = 4, kRowIters = 8, kRowState = 16, kRowHeur = 32, kRowFlags = 64 };

unsigned rows_of(const mplx_succ_lists *o) {
  return (o->action ? kRowAction : 0u) | (o->cost ? kRowCost : 0u) | (o->hash ? kRowHash : 0u) |
         (o->iters ? kRowIters : 0u) | (o->state ? kRowState : 0u) | (o->heur ? kRowHeur : 0u) | (o->flags ? kRowFlags : 0u);
}

ArenaLayout arena_layout(int F, int64_t n_alloc, int64_t S, unsigned rows) {
  ArenaLayout L;
  L.n_alloc = n_alloc;
  L.n_slots = n_alloc * S;
  L.o_count = align256((size_t)F * n_alloc * 8);
  L.o_action = L.o_count + align256((size_t)n_alloc * 4);
  L.o_cost = L.o_action + ((rows & kRowAction) ? align256((size_t)L.n_slots * 4) : 0);
  L.o_hash = L.o_cost + ((rows & kRowCost) ? align256((size_t)L.n_slots * 8) : 0);
  L.o_iters = L.o_hash + ((rows & kRowHash) ? align256((size_t)L.n_slots * 8) : 0);
  L.o_heur = L.o_iters + ((rows & kRowIters) ? align256((size_t)L.n_slots * 4) : 0);
  L.o_flags = L.o_heur + ((rows & kRowHeur) ? align256((size_t)L.n_slots * 8) : 0);
  L.o_state = L.o_flags + ((rows & kRowFlags) ? align256((size_t)L.n_slots) : 0);
  L.total = L.o_state + ((rows & kRowState) ? align256((size_t)F * L.n_slots * 8) : 0);
  return L;
}

void arena_put_nodes(char *hb, const ArenaLayout &L, int F, const double *h_nodes, int64_t n_nodes, int64_t node_stride) {
  for (int f = 0; f < F; f++)
    std::memcpy(hb + (size_t)f * L.n_alloc * 8, h_nodes + (size_t)f * node_stride, (size_t)n_nodes * 8);
}

mplx_succ_lists arena_lists(char *b, const ArenaLayout &L, int64_t S, unsigned rows) {
  mplx_succ_lists d{};
  d.count = (int32_t *)(b + L.o_count);
  if (rows & kRowAction) d.action = (int32_t *)(b + L.o_action);
  if (rows & kRowCost) d.cost = (double *)(b + L.o_cost);
  if (rows & kRowHash) d.hash = (uint64_t *)(b + L.o_hash);
  if (rows & kRowIters) d.iters = (int32_t *)(b + L.o_iters);
  if (rows & kRowHeur) d.heur = (double *)(b + L.o_heur);
  if (rows & kRowFlags) d.flags = (uint8_t *)(b + L.o_flags);
  if (rows & kRowState) { d.state = (double *)(b + L.o_state); d.state_stride = L.n_slots; }
  d.node_stride = S;
  return d;
}

// the used prefix of every list, from the landing block into the caller's arrays
void arena_get_lists(const char *hb, const ArenaLayout &L, int F, int64_t S, int64_t n_nodes, const mplx_succ_lists *h_out) {
  const int32_t *cnt = (const int32_t *)(hb + L.o_count);
  std::memcpy(h_out->count, cnt, (size_t)n_nodes * 4);
  for (int64_t k = 0; k < n_nodes; k++) {
    const size_t m = (size_t)cnt[k], at = (size_t)k * (size_t)S;
    if (!m) continue;
    if (h_out->action) std::memcpy(h_out->action + at, hb + L.o_action + at * 4, m * 4);
    if (h_out->cost) std::memcpy(h_out->cost + at, hb + L.o_cost + at * 8, m * 8);
    if (h_out->hash) std::memcpy(h_out->hash + at, hb + L.o_hash + at * 8, m * 8);
    if (h_out->iters) std::memcpy(h_out->iters + at, hb + L.o_iters + at * 4, m * 4);
    if (h_out->heur) std::memcpy(h_out->heur + at, hb + L.o_heur + at * 8, m * 8);
    if (h_out->flags) std::memcpy(h_out->flags + at, hb + L.o_flags + at, m);
    if (h_out->state)
      for (int f = 0; f < F; f++)
        std::memcpy(h_out->state + (size_t)f * h_out->state_stride + at,
                    hb + L.o_state + ((size_t)f * L.n_slots + at) * 8, m * 8);
  }
}

// (Re)launch the resident kernel with the signature in c->svc (cap, S, rows); seq_served = the last request that
// has been answered.  The context's own stream is drained
// first: the resident kernel runs on a stream of its own and reads what earlier calls uploaded.
int svc_launch(mplx_ctx *c, const TilePlan &tp, uint32_t seq_served) {
  mplx_ctx::Service &sv = c->svc;
  const int F = 4 * c->dim + 2;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!sv.stream) HIP_TRY(c, hipStreamCreateWithFlags(&sv.stream, hipStreamNonBlocking));
  if (!sv.mb) {
    HIP_TRY(c, hipHostMalloc((void **)&sv.mb, sizeof(mplx::SvcMailbox), hipHostMallocCoherent));
    std::memset(sv.mb, 0, sizeof(mplx::SvcMailbox));
  }
  if (int rc = ensure_tables(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const ArenaLayout L = arena_layout(F, sv.cap, sv.S, sv.rows);
  if (L.total > sv.block_cap) {
    if (sv.block) HIP_TRY(c, hipHostFree(sv.block));
    sv.block = nullptr;
    sv.block_cap = 0;
    HIP_TRY(c, hipHostMalloc((void **)&sv.block, L.total, hipHostMallocCoherent));
    sv.block_cap = L.total;
  }
  int64_t g = (sv.cap + tp.npb - 1) / tp.npb;
  if (g > tp.grid) g = tp.grid;  // every workgroup must be resident: each waits for the others
  if (g > 1024) g = 1024;
  sv.workgroups = (int)g;
  if (int rc = ensure(c, sv.dev, (size_t)(1 + g) * 8)) return rc;
  HIP_TRY(c, hipMemsetAsync(sv.dev.p, 0, (size_t)(1 + g) * 8, sv.stream));
  const mplx_succ_lists d = arena_lists(sv.block, L, sv.S, sv.rows);
  mplx::TileArgs a = tile_args(c, tp, (const double *)sv.block, sv.cap, sv.cap, &d);
  a.grid_limit = (int32_t)g;
  a.svc_mb = sv.mb;
  a.svc_dev = (uint64_t *)sv.dev.p;
  a.svc_seq0 = seq_served;  // the kernel waits for the request after this one
  a.svc_idle = (uint64_t)c->tune.service_idle_us * 100ull;  // ticks of the 100 MHz clock
  // every workgroup of the resident form waits for the others: the runtime's own occupancy figure has to cover the grid
  // (tp.grid is an LDS estimate; a register-limited instantiation or a smaller device would otherwise hang the handshake
  // until the 2 s give-up).  Fewer than asked for: this context serves its small batches with launches.
  const int resident = mplx::tile_service_resident_workgroups(c->dim, c->prm.control, a);
  if (resident > 0 && resident < (int)g) {
    sv.disabled = true;
    return MPLX_OK;
  }
  *(volatile uint32_t *)&sv.mb->quit = 0;
  *(volatile uint32_t *)&sv.mb->alive = 1;
  std::atomic_thread_fence(std::memory_order_seq_cst);
  HIP_TRY(c, mplx::launch_expand_tile(c->dim, c->prm.control, a, sv.stream));
  sv.running = true;
  sv.launches++;
  return MPLX_OK;
}
}  // namespace

int mplx_detail::svc_stop(mplx_ctx *c) {
  mplx_ctx::Service &sv = c->svc;
  if (!sv.running) return MPLX_OK;
  sv.running = false;
  *(volatile uint32_t *)&sv.mb->quit = 1;  // the coordinator polls this word between requests
  std::atomic_thread_fence(std::memory_order_seq_cst);
  const hipError_t e = hipStreamSynchronize(sv.stream);
  *(volatile uint32_t *)&sv.mb->quit = 0;
  if (e != hipSuccess) {
    sv.disabled = true;
    return fail(c, MPLX_ERR_HIP, "the resident expansion kernel did not leave: %s", hipGetErrorString(e));
  }
  return MPLX_OK;
}

int mplx_detail::wait_small_launch(mplx_ctx *c) {
  if (!c->done_armed) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MPLX_OK;
  }
  c->done_armed = false;
  volatile uint64_t *f = c->done_host;
  const uint64_t want = c->done_seq;
  double t0 = 0;
  c->done_waits++;
  for (uint32_t spins = 1; *f != want; spins++) {
    __builtin_ia32_pause();
    if ((spins & 0xfffu) != 0) continue;
    const double now = mono_us();
    if (t0 == 0) t0 = now;
    if (now - t0 > 2e5) {  // 200 ms: the word did not come -- the stream decides, and this context stops asking for it
      c->done_timeouts++;
      c->tune.done_flag = 0;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      (void)hipMemsetAsync(c->done_count.p, 0, 64, c->stream);
      return MPLX_OK;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return MPLX_OK;
}

// One small batch through the resident kernel.  *handled = false: not this time (not eligible, or the service gave
// up) -- the caller runs the batch as a launch of its own.  h_out names the rows (and the list stride) wanted; the
// used prefixes are copied into its arrays, or, with `view`, left in the landing block and described there (row stride
// view->state_stride = capacity x list stride).
int mplx_detail::svc_request(mplx_ctx *c, const double *h_nodes, int64_t n_nodes, int64_t node_stride, const mplx_succ_lists *h_out,
                bool *handled, mplx_succ_lists *view) {
  *handled = false;
  mplx_ctx::Service &sv = c->svc;
  if (!c->tune.service || sv.disabled) return MPLX_OK;
  const TilePlan tp = (c->lists_route == MPLX_ROUTE_AUTO || c->lists_route == MPLX_ROUTE_TILE) ? plan_tile(c) : TilePlan();
  // (more than 64 workgroups in the handshake cost more than they save: 256 nodes of the 729-control table, a
  // workgroup each, 88 us per request against 65 us as a launch; 64 nodes 30 against 41)
  constexpr int64_t kMaxWorkgroups = 64;
  if (!tp.ok || n_nodes > c->tune.service_max_nodes || (n_nodes + tp.npb - 1) / tp.npb > kMaxWorkgroups) {
    // not a search's batch: the row of such batches ends here
    sv.streak = 0;
    return MPLX_OK;
  }
  const int F = 4 * c->dim + 2;
  const int64_t S = list_stride(c, h_out);
  const unsigned rows = rows_of(h_out);
  if (!sv.running || S != sv.S || (rows & ~sv.rows) != 0 || n_nodes > sv.cap) {
    if (!sv.running && ++sv.streak < 2) return MPLX_OK;  // a single call is not a search
    if (int rc = svc_stop(c)) return rc;
    int64_t cap = 64;
    while (cap < n_nodes) cap <<= 1;
    const size_t arena_max = c->tune.arena_kb > 0 ? (size_t)c->tune.arena_kb << 10 : (size_t)8 << 20;
    const unsigned want_rows = (S == sv.S) ? (rows | sv.rows) : rows;
    while (cap > n_nodes && (arena_layout(F, cap, S, want_rows).total > arena_max || (cap + tp.npb - 1) / tp.npb > kMaxWorkgroups)) cap >>= 1;
    if (cap < n_nodes) cap = n_nodes;
    if (arena_layout(F, cap, S, want_rows).total > arena_max) return MPLX_OK;
    sv.cap = cap;
    // (callers that alternate between two sets of rows -- a search's batches and single get_succ calls -- get the union,
    // not a restart per call)
    sv.rows = (S == sv.S) ? (rows | sv.rows) : rows;
    sv.S = S;
    if (sv.seq > 0xfffffff0u) {  // (the doorbell of the last request still carries the old number)
      sv.seq = 0;
      if (sv.mb) *(volatile uint64_t *)&sv.mb->doorbell = 0;
    }
    if (int rc = svc_launch(c, tp, sv.seq)) return rc;
    if (!sv.running) return MPLX_OK;  // (not resident on this device: see svc_launch)
  }
  const ArenaLayout L = arena_layout(F, sv.cap, sv.S, sv.rows);
  arena_put_nodes(sv.block, L, F, h_nodes, n_nodes, node_stride);
  const uint32_t seq = ++sv.seq;
  std::atomic_thread_fence(std::memory_order_release);
  *(volatile uint64_t *)&sv.mb->doorbell = ((uint64_t)seq << 32) | (uint64_t)(uint32_t)n_nodes;
  volatile uint64_t *done = &sv.mb->done;
  volatile uint32_t *alive = &sv.mb->alive;
  double t0 = 0;
  int relaunches = 0;
  for (uint32_t spins = 1; *done != (uint64_t)seq; spins++) {
    __builtin_ia32_pause();
    if ((spins & 0x3ffu) != 0) continue;
    const double now = mono_us();
    if (t0 == 0) t0 = now;
    if (*alive == 0 && *done != (uint64_t)seq && relaunches < 2) {
      // the kernel left (no request for service_idle_us) before it saw this one: the next one picks it up
      sv.running = false;
      relaunches++;
      if (int rc = svc_launch(c, tp, seq - 1)) return rc;
      if (!sv.running) return MPLX_OK;
    } else if (now - t0 > 2e6) {
      // no answer: give the batch to an ordinary launch and never try again in this context
      sv.failures++;
      (void)svc_stop(c);
      sv.disabled = true;
      return MPLX_OK;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  if (view) *view = arena_lists(sv.block, L, sv.S, sv.rows);  // the lists where they landed (valid until the next call)
  else arena_get_lists(sv.block, L, F, sv.S, n_nodes, h_out);
  sv.requests++;
  c->last_route = MPLX_ROUTE_TILE;
  *handled = true;
  return MPLX_OK;
}

extern "C" {

int mplx_expand_lists(mplx_ctx *c, const double *h_nodes, int64_t n_nodes, int64_t node_stride,
                      const mplx_succ_lists *h_out) {
  if (!c) return MPLX_ERR_ARG;
  if (!h_out || !h_out->count || n_nodes < 0 || node_stride < n_nodes || (!h_nodes && n_nodes > 0))
    return fail(c, MPLX_ERR_ARG, "mplx_expand_lists: bad arguments");
  if (int rc = ctx_ready(c)) return rc;
  if (n_nodes == 0) return MPLX_OK;
  const int F = 4 * c->dim + 2;
  if (h_out->node_stride != 0 && h_out->node_stride < c->nU)
    return fail(c, MPLX_ERR_ARG, "mplx_expand_lists: node_stride %lld < nU %d", (long long)h_out->node_stride, c->nU);
  const int64_t S = list_stride(c, h_out), n_slots = n_nodes * S;
  if (h_out->state && h_out->state_stride < n_slots)
    return fail(c, MPLX_ERR_ARG, "mplx_expand_lists: state_stride < n_nodes*node_stride");
  {
    // The batches of a search (a few nodes, the answer awaited before the next one is known) go through a kernel
    // that stays resident between them, from the second such call in a row: a mailbox round trip instead of launch +
    // synchronise (see expand_tile_kernel.hip, SERVICE MODE).  Any other call into the context ends it (bind_device).
    bool handled = false;
    if (int rc = svc_request(c, h_nodes, n_nodes, node_stride, h_out, &handled, nullptr)) return rc;
    if (handled) return MPLX_OK;
    const int counted = c->svc.streak;  // (what svc_request made of it; bind_device resets it)
    if (int rc = bind_device(c)) return rc;
    c->svc.streak = counted;
  }
  {
    // Small batches (one get_succ, or the speculative batches of a search) are latency bound: nodes and every
    // output row live in ONE pinned host block that the kernel reads and writes itself over PCIe (only the used
    // list entries cross the link, while the kernel runs), so a call is the kernel and one synchronisation; the
    // used prefixes are then copied into the caller's arrays.  (A 2D 9-control get_succ: 25 us; with one pageable
    // copy per row 111 us, with one upload + one download through a device arena 28 us -- MPLX_ZERO_COPY=0.)
    const unsigned rows = rows_of(h_out);
    const ArenaLayout L = arena_layout(F, n_nodes, S, rows);
    const size_t total = L.total, o_count = L.o_count;
    const size_t arena_max = c->tune.arena_kb > 0 ? (size_t)c->tune.arena_kb << 10 : (size_t)8 << 20;
    if (total <= arena_max) {
      if (int rc = ensure(c, c->s_arena, total)) return rc;
      if (total > c->h_arena_cap) {
        if (c->h_arena) HIP_TRY(c, hipHostFree(c->h_arena));
        c->h_arena = nullptr;
        c->h_arena_cap = 0;
        HIP_TRY(c, hipHostMalloc(&c->h_arena, arena_max, hipHostMallocCoherent));  // read by the host while the kernel may still run (DoneSignal)
        c->h_arena_cap = arena_max;
      }
      char *hb = (char *)c->h_arena, *db = (char *)c->s_arena.p;
      arena_put_nodes(hb, L, F, h_nodes, n_nodes, node_stride);
      const bool zero_copy = c->tune.zero_copy != 0;
      if (zero_copy) db = hb;  // the kernel reads the nodes from and writes the lists to the pinned host block itself
      else HIP_TRY(c, hipMemcpyAsync(db, hb, (size_t)F * n_nodes * 8, hipMemcpyHostToDevice, c->stream));
      const mplx_succ_lists d = arena_lists(db, L, h_out->node_stride, rows);
      c->want_done = zero_copy;  // the kernel tells the host itself when the lists are in the block (DoneSignal)
      const int rc_launch = lists_device(c, (const double *)db, n_nodes, n_nodes, &d);
      c->want_done = false;
      if (rc_launch) return rc_launch;
      if (!zero_copy)
        HIP_TRY(c, hipMemcpyAsync(hb + o_count, db + o_count, total - o_count, hipMemcpyDeviceToHost, c->stream));
      if (int rc = wait_small_launch(c)) return rc;
      if (!c->yaw_pending.empty()) {  // a fix pass of the yaw pinning rewrites lists on the device side
        if (int rc = resolve_pending(c, true)) return rc;
        if (!zero_copy) {
          HIP_TRY(c, hipMemcpyAsync(hb + o_count, db + o_count, total - o_count, hipMemcpyDeviceToHost, c->stream));
          HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
      }
      arena_get_lists(hb, L, F, S, n_nodes, h_out);
      return MPLX_OK;
    }
  }
  if (h_out->heur || h_out->flags)
    return fail(c, MPLX_ERR_ARG, "mplx_expand_lists: the heur / flags rows come back through host pointers for batches of up to "
                                 "8 MiB of lists only (a search's); larger ones: mplx_expand_lists_device and a copy of the rows");
  const size_t slots = (size_t)n_slots;
  StageLayout l;
  const size_t o_nodes = l.add((size_t)F * n_nodes * 8), o_count = l.add((size_t)n_nodes * 4), o_action = l.add(h_out->action ? slots * 4 : 0),
               o_cost = l.add(h_out->cost ? slots * 8 : 0), o_hash = l.add(h_out->hash ? slots * 8 : 0),
               o_iters = l.add(h_out->iters ? slots * 4 : 0), o_state = l.add(h_out->state ? F * slots * 8 : 0);
  if (int rc = stage_commit(c, &l)) return rc;
  HIP_TRY(c, stage_in_rows(c, l.base + o_nodes, h_nodes, (size_t)node_stride * 8, (size_t)n_nodes * 8, F));
  mplx_succ_lists d{};
  d.count = (int32_t *)(l.base + o_count);
  if (h_out->action) d.action = (int32_t *)(l.base + o_action);
  if (h_out->cost) d.cost = (double *)(l.base + o_cost);
  if (h_out->hash) d.hash = (uint64_t *)(l.base + o_hash);
  if (h_out->iters) d.iters = (int32_t *)(l.base + o_iters);
  if (h_out->state) { d.state = (double *)(l.base + o_state); d.state_stride = n_slots; }
  d.node_stride = h_out->node_stride;
  if (int rc = lists_device(c, (const double *)(l.base + o_nodes), n_nodes, n_nodes, &d)) return rc;
  // everything larger: only the used prefixes cross the link, packed on the device and pipelined through pinned
  // buffers (lists_copy_api.cpp); that copy returns with the stream idle: nothing reads the arena after this call
  MPLX_GUARD_BEGIN
  if (int rc = resolve_pending(c)) return rc;
  return copy_lists_to_host(c, d, h_out, n_nodes);
  MPLX_GUARD_END(c)
}

int mplx_get_succ(mplx_ctx *c, const double *node, double *succ, double *cost, int32_t *action,
                  int32_t *n_succ) {
  if (!c) return MPLX_ERR_ARG;
  if (!node || !succ || !cost || !action || !n_succ) return fail(c, MPLX_ERR_ARG, "mplx_get_succ: NULL argument");
  if (int rc = ctx_ready(c)) return rc;
  MPLX_GUARD_BEGIN
  const int F = 4 * c->dim + 2;
  const int nU = c->nU;
  c->h_state.resize((size_t)F * nU);
  int32_t count = 0;
  mplx_succ_lists o{};
  o.count = &count;
  o.action = action;
  o.cost = cost;
  o.state = c->h_state.data();
  o.state_stride = nU;
  if (int rc = mplx_expand_lists(c, node, 1, 1, &o)) return rc;
  for (int m = 0; m < count; m++)
    for (int f = 0; f < F; f++) succ[(size_t)m * F + f] = c->h_state[(size_t)f * nU + m];
  *n_succ = count;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

int mplx_service(mplx_ctx *c, int mode, int64_t stats[4]) {
  if (!c) return MPLX_ERR_ARG;
  if (mode < -1 || mode > 1) return fail(c, MPLX_ERR_ARG, "mplx_service: mode must be -1, 0 or 1");
  if (mode >= 0) {
    c->tune.service = mode;
    c->svc.streak = 0;
    if (mode == 0) {
      if (int rc = svc_stop(c)) return rc;
    }
  }
  if (stats) {
    stats[0] = c->svc.requests;
    stats[1] = c->svc.launches;
    stats[2] = c->svc.failures;
    stats[3] = c->svc.running ? 1 : 0;
  }
  return MPLX_OK;
}

}  // extern "C"
