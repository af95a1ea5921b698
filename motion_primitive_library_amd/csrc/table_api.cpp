// table_api.cpp -- C ABI of include/mplx_table.h: the persistent node table on the device (table_kernel.hip).  The
// table's arrays, its control block and its scratch are the table's own; launches go to the context's stream and the
// host-pointer calls stage through the context's arena.
#include "mplx_ctx.h"
#include "../../include/mplx_multi.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace mplx_detail;

struct mplx_table {
  mplx_ctx *c = nullptr;
  int64_t cap = 0;
  uint64_t n_slots = 0;              // all regions together (the dedicated slots of the empty marker come behind them)
  uint64_t q_slots = 0;              // one query's region
  int32_t Q = 1;
  int F = 0;
  DevBuf slots, hash, g, pred, pact, state, pick, ctl;
  DevBuf query;                      // per node its query: tables with Q > 1 only
  DevBuf scratch;                    // per-call passes (ent, mark, tile counts, seed hashes); grows on demand
  DevBuf replan;                     // the passes of a rebase (replan_kernel.hip), for `cap` nodes; allocated by the first rebase
  mplx::TableMirror *mirror = nullptr;  // pinned
  uint32_t epoch = 0;                // calls since the last clear
  int64_t bound = 0;                 // upper bound of n_nodes: the mirror's value at the last wait + what the calls queued since can add
  bool poisoned = false;             // the host has seen a status bit
  bool time_keys = false;            // mplx_table_set_time_keys: a node's key is hash_combine(hash, (int)round(t / 0.1))
};

namespace {

constexpr int64_t kMaxEntries = 0x7ffffffeLL;  // e and the "no entry" word share 32 bits

mplx::TableArgs table_args(const mplx_table *t) {
  mplx::TableArgs a{};
  a.slots = (mplx::TableSlot *)t->slots.p;
  a.n_slots = t->n_slots;
  a.q_slots = t->q_slots;
  a.n_queries = t->Q;
  a.query = (int32_t *)t->query.p;
  a.hash = (uint64_t *)t->hash.p;
  a.g = (unsigned long long *)t->g.p;
  a.pred = (int32_t *)t->pred.p;
  a.pred_action = (int32_t *)t->pact.p;
  a.state = (double *)t->state.p;
  a.pick = (unsigned long long *)t->pick.p;
  a.cap = t->cap;
  a.n_fields = t->F;
  a.ctl = (mplx::TableCtl *)t->ctl.p;
  a.mirror = t->mirror;
  return a;
}

void release_table(mplx_table *t) {
  for (DevBuf *b : {&t->slots, &t->hash, &t->g, &t->pred, &t->pact, &t->state, &t->pick, &t->ctl, &t->query, &t->scratch, &t->replan}) release(*b);
  if (t->mirror) (void)hipHostFree(t->mirror);
  delete t;
}

int usable(mplx_table *t, const char *who) {
  if (t->poisoned)
    return fail(t->c, MPLX_ERR_STATE, "%s: the table has status %u (1 nodes full, 2 probe full, 4 frontier full): mplx_table_clear first", who,
                (unsigned)t->mirror->status);
  return MPLX_OK;
}

// after a wait for the stream: what the last finished call left
void observe(mplx_table *t) {
  if (*(volatile uint32_t *)&t->mirror->status) t->poisoned = true;
  else t->bound = *(volatile int64_t *)&t->mirror->n_nodes;
}

int check_frontier(mplx_ctx *c, const char *who, const mplx_table_frontier *f) {
  if (!f || !f->id || !f->g || !f->state || !f->count || f->capacity < 0 || f->state_stride < f->capacity)
    return fail(c, MPLX_ERR_ARG, "%s: the frontier needs id, g, state and count, and state_stride >= capacity >= 0", who);
  return MPLX_OK;
}

// The passes of one call over n_rows * S entries; `seed_hashes` more bytes of scratch in front for a seed's hashes.
// With time keys one more row of n keys, which the passes then read as the entries' hashes (*keys_out).
int run_passes(mplx_table *t, mplx::TableArgs *a, const mplx_table_frontier *f, size_t seed_hashes, void **seed_hash_out,
               uint64_t **keys_out = nullptr) {
  mplx_ctx *c = t->c;
  const int64_t n = a->n_rows * a->S;
  a->n_tiles = (n + mplx::kTableTile - 1) / mplx::kTableTile;
  StageLayout l;  // (only the carving: the table's own scratch, not the arena)
  const size_t o_h = l.add(seed_hashes), o_ent = l.add((size_t)n * 4), o_mark = l.add((size_t)n), o_tot = l.add((size_t)a->n_tiles * 4),
               o_key = l.add(keys_out ? (size_t)n * 8 : 0);
  if (int rc = ensure(c, t->scratch, l.total)) return rc;
  char *base = (char *)t->scratch.p;
  if (seed_hash_out) *seed_hash_out = base + o_h;
  if (keys_out) *keys_out = (uint64_t *)(base + o_key);
  a->ent = (uint32_t *)(base + o_ent);
  a->mark = (uint8_t *)(base + o_mark);
  a->tot = (uint32_t *)(base + o_tot);
  a->f_id = f->id; a->f_g = f->g; a->f_state = f->state; a->f_stride = f->state_stride; a->f_cap = f->capacity; a->f_count = f->count;
  if (t->epoch >= 0xfffffff0u) return fail(c, MPLX_ERR_STATE, "mplx_table: 2^32 calls since the last mplx_table_clear");
  t->epoch++;
  a->tag = 0xffffffffu - t->epoch;
  t->bound = std::min(t->cap, t->bound + n);  // every entry may be a new node
  return MPLX_OK;
}

int read_count(mplx_table *t, const mplx_table_frontier *f, int64_t *h_count) {
  mplx_ctx *c = t->c;
  HIP_TRY(c, hipMemcpyAsync(h_count, f->count, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  observe(t);
  return MPLX_OK;
}

}  // namespace

// What the open set of a table (open_api.cpp) needs of it.
namespace mplx_detail {

int table_open_args(mplx_table *t, const char *who, mplx_ctx **c, mplx::OpenArgs *a) {
  *c = t->c;
  if (int rc = usable(t, who)) return rc;
  a->t_ctl = (const mplx::TableCtl *)t->ctl.p;
  a->t_hash = (const uint64_t *)t->hash.p;
  a->t_g = (const unsigned long long *)t->g.p;
  a->t_state = (const double *)t->state.p;
  a->t_query = (const int32_t *)t->query.p;
  a->n_queries = t->Q;
  a->cap = t->cap;
  a->n_fields = t->F;
  a->n_bound = t->bound;
  return MPLX_OK;
}

void table_observe(mplx_table *t) { observe(t); }

int table_replan_args(mplx_table *t, const char *who, bool scratch, mplx_ctx **c, mplx::ReplanArgs *a, int32_t *time_keys) {
  *c = t->c;
  if (int rc = usable(t, who)) return rc;
  if (time_keys) *time_keys = t->time_keys ? 1 : 0;
  else if (t->time_keys) return fail(t->c, MPLX_ERR_STATE, "%s: the table has time keys (mplx_table_set_time_keys): it cannot be rebased (mplx_table_rebase_timed_device can)", who);
  a->n_queries = t->Q;
  a->n_bound = t->bound;
  if (!scratch) return MPLX_OK;
  const size_t cap = (size_t)t->cap, tiles = (cap + mplx::kTableTile - 1) / mplx::kTableTile;
  StageLayout l;  // (only the carving: the table's own scratch, not the arena)
  const size_t o_bad = l.add(cap), o_d0 = l.add(cap), o_d1 = l.add(cap), o_j0 = l.add(cap * 4), o_j1 = l.add(cap * 4), o_mark = l.add(cap),
               o_tot = l.add(tiles * 4), o_cnt = l.add(sizeof(mplx::ReplanResult));
  if (int rc = ensure(t->c, t->replan, l.total)) return rc;
  char *base = (char *)t->replan.p;
  a->bad = (uint8_t *)(base + o_bad);
  a->dec[0] = (uint8_t *)(base + o_d0);
  a->dec[1] = (uint8_t *)(base + o_d1);
  a->jump[0] = (int32_t *)(base + o_j0);
  a->jump[1] = (int32_t *)(base + o_j1);
  a->mark = (uint8_t *)(base + o_mark);
  a->tot = (uint32_t *)(base + o_tot);
  a->counters = (mplx::ReplanResult *)(base + o_cnt);
  a->ctl = (mplx::TableCtl *)t->ctl.p;
  a->mirror = t->mirror;
  a->hash = (const uint64_t *)t->hash.p;
  a->g = (unsigned long long *)t->g.p;
  a->pred = (int32_t *)t->pred.p;
  a->pred_action = (int32_t *)t->pact.p;
  a->state = (const double *)t->state.p;
  a->query = (const int32_t *)t->query.p;
  a->n_queries = t->Q;
  a->n_fields = t->F;
  a->cap = t->cap;
  a->n_bound = t->bound;
  return MPLX_OK;
}

int table_reserve_args(mplx_table *t, const char *who, mplx_ctx **c, const int32_t **d_query, int32_t *n_queries, int64_t *cap) {
  *c = t->c;
  if (int rc = usable(t, who)) return rc;
  *d_query = (const int32_t *)t->query.p;
  *n_queries = t->Q;
  *cap = t->cap;
  return MPLX_OK;
}

}  // namespace mplx_detail

namespace {

// Q regions of q_slots slots each; the arguments are checked
int create_table(mplx_ctx *c, const char *who, int64_t node_capacity, int32_t Q, uint64_t q_slots, mplx_table **out) {
  *out = nullptr;
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  mplx_table *t = new mplx_table;
  t->c = c;
  t->cap = node_capacity;
  t->Q = Q;
  t->q_slots = q_slots;
  t->n_slots = q_slots * (uint64_t)Q;
  t->F = 4 * c->dim + 2;
  const uint64_t n_slots = t->n_slots;
  const size_t cap = (size_t)node_capacity;
  int rc = MPLX_OK;
  if (!rc) rc = ensure(c, t->slots, (size_t)(n_slots + (uint64_t)Q) * sizeof(mplx::TableSlot));
  if (!rc && Q > 1) rc = ensure(c, t->query, cap * 4);
  if (!rc) rc = ensure(c, t->hash, cap * 8);
  if (!rc) rc = ensure(c, t->g, cap * 8);
  if (!rc) rc = ensure(c, t->pred, cap * 4);
  if (!rc) rc = ensure(c, t->pact, cap * 4);
  if (!rc) rc = ensure(c, t->state, cap * 8 * (size_t)t->F);
  if (!rc) rc = ensure(c, t->pick, cap * 8);
  if (!rc) rc = ensure(c, t->ctl, sizeof(mplx::TableCtl));
  if (!rc && hipHostMalloc((void **)&t->mirror, 64, hipHostMallocCoherent) != hipSuccess)
    rc = fail(c, MPLX_ERR_HIP, "%s: hipHostMalloc failed", who);
  if (!rc && mplx::launch_table_clear(table_args(t), c->stream) != hipSuccess) rc = fail(c, MPLX_ERR_HIP, "%s: the clearing launch failed", who);
  if (rc) {
    (void)hipGetLastError();
    release_table(t);
    return rc;
  }
  *out = t;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

// what the plain calls answer on a table with several queries
int single_only(mplx_table *t, const char *who) {
  if (t->Q > 1) return fail(t->c, MPLX_ERR_STATE, "%s: the table has %d queries: use the _multi form (mplx_multi.h)", who, (int)t->Q);
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_table_create(mplx_ctx *c, int64_t node_capacity, int32_t slots_log2, mplx_table **out) {
  if (!c) return MPLX_ERR_ARG;
  if (!out || node_capacity < 1 || node_capacity >= (1LL << 31) || slots_log2 < 0 || slots_log2 > 31)
    return fail(c, MPLX_ERR_ARG, "mplx_table_create: need out, 1 <= node_capacity < 2^31 and 0 <= slots_log2 <= 31");
  uint64_t n_slots = 0;
  if (slots_log2 == 0) {
    n_slots = 2;
    while (n_slots < 2 * (uint64_t)node_capacity && n_slots < (1ull << 31)) n_slots <<= 1;
  } else {
    n_slots = 1ull << slots_log2;
  }
  if (n_slots <= (uint64_t)node_capacity)
    return fail(c, MPLX_ERR_ARG, "mplx_table_create: 2^slots_log2 = %llu slots cannot hold %lld nodes", (unsigned long long)n_slots, (long long)node_capacity);
  return create_table(c, "mplx_table_create", node_capacity, 1, n_slots, out);
}

int mplx_table_create_multi(mplx_ctx *c, int64_t node_capacity, int32_t n_queries, int32_t query_slots_log2, mplx_table **out) {
  if (!c) return MPLX_ERR_ARG;
  const char *who = "mplx_table_create_multi";
  if (n_queries == 1) return mplx_table_create(c, node_capacity, query_slots_log2, out);  // the same table
  if (!out || node_capacity < 1 || node_capacity >= (1LL << 31) || query_slots_log2 < 0 || query_slots_log2 > 31)
    return fail(c, MPLX_ERR_ARG, "%s: need out, 1 <= node_capacity < 2^31 and 0 <= query_slots_log2 <= 31", who);
  if (n_queries < 1 || n_queries > 65536) return fail(c, MPLX_ERR_ARG, "%s: n_queries = %d is not in [1, 65536]", who, (int)n_queries);
  uint64_t q_slots = 0;
  if (query_slots_log2 == 0) {
    const uint64_t share = ((uint64_t)node_capacity + (uint64_t)n_queries - 1) / (uint64_t)n_queries;
    q_slots = 64;
    while (q_slots < 2 * share) q_slots <<= 1;
  } else {
    q_slots = 1ull << query_slots_log2;
  }
  // slot indices are uint32 in the per-entry scratch, 2^32 - 1 means "none", and the dedicated slots come last
  if (q_slots * (uint64_t)n_queries + (uint64_t)n_queries >= 0xffffffffull)
    return fail(c, MPLX_ERR_ARG, "%s: %d regions of %llu slots exceed the 32-bit slot index", who, (int)n_queries, (unsigned long long)q_slots);
  return create_table(c, who, node_capacity, n_queries, q_slots, out);
}

int mplx_table_query_of(mplx_table *t, const int32_t **d_query, int32_t *n_queries) {
  if (!t) return MPLX_ERR_ARG;
  if (!d_query && !n_queries) return fail(t->c, MPLX_ERR_ARG, "mplx_table_query_of: nothing asked for");
  if (d_query) *d_query = (const int32_t *)t->query.p;
  if (n_queries) *n_queries = t->Q;
  return MPLX_OK;
}

void mplx_table_destroy(mplx_table *t) {
  if (!t) return;
  (void)hipSetDevice(t->c->device);
  (void)hipStreamSynchronize(t->c->stream);
  release_table(t);
}

int mplx_table_clear(mplx_table *t) {
  if (!t) return MPLX_ERR_ARG;
  mplx_ctx *c = t->c;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, mplx::launch_table_clear(table_args(t), c->stream));
  t->epoch = 0;
  t->poisoned = false;
  t->bound = 0;
  return MPLX_OK;
}

int mplx_table_set_time_keys(mplx_table *t, int32_t on) {
  if (!t) return MPLX_ERR_ARG;
  if (t->epoch != 0 || t->bound != 0)
    return fail(t->c, MPLX_ERR_STATE, "mplx_table_set_time_keys: the table is not empty: only after mplx_table_create or mplx_table_clear");
  t->time_keys = on != 0;
  return MPLX_OK;
}

uint64_t mplx_time_key(uint64_t hash, double t) {
  const int id = (int)std::round(t / 0.1);  // waypoint.h:119-122
  return hash ^ ((uint64_t)(int64_t)id + 0x9e3779b9ULL + (hash << 6) + (hash >> 2));
}

int mplx_table_view_of(mplx_table *t, mplx_table_view *v) {
  if (!t) return MPLX_ERR_ARG;
  if (!v) return fail(t->c, MPLX_ERR_ARG, "mplx_table_view_of: NULL view");
  v->hash = (const uint64_t *)t->hash.p;
  v->g = (const double *)t->g.p;
  v->pred = (const int32_t *)t->pred.p;
  v->pred_action = (const int32_t *)t->pact.p;
  v->state = (const double *)t->state.p;
  v->state_stride = t->cap;
  return MPLX_OK;
}

int mplx_table_stats(mplx_table *t, int64_t *n_nodes, uint32_t *status) {
  if (!t) return MPLX_ERR_ARG;
  mplx_ctx *c = t->c;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  observe(t);
  if (n_nodes) *n_nodes = *(volatile int64_t *)&t->mirror->n_nodes;
  if (status) *status = *(volatile uint32_t *)&t->mirror->status;
  return MPLX_OK;
}

int mplx_table_relax_device(mplx_table *t, const mplx_succ_lists *L, int64_t n_nodes, const int32_t *d_parent_id,
                            const double *d_parent_g, double g_max, const mplx_table_frontier *d_next, int32_t *d_entry_id,
                            int64_t *h_count) {
  if (!t) return MPLX_ERR_ARG;
  mplx_ctx *c = t->c;
  const char *who = "mplx_table_relax_device";
  if (!L || n_nodes < 0 || !d_parent_id || !d_parent_g) return fail(c, MPLX_ERR_ARG, "%s: NULL argument or n_nodes < 0", who);
  if (int rc = check_frontier(c, who, d_next)) return rc;
  if (!L->count || !L->hash || !L->cost || !L->action || !L->state)
    return fail(c, MPLX_ERR_ARG, "%s: the lists need count, action, cost, hash and state", who);
  const int64_t S = list_stride(c, L);
  if (S < 1 || n_nodes > kMaxEntries / S) return fail(c, MPLX_ERR_ARG, "%s: node_stride < 1 or more than 2^31 - 2 list entries", who);
  if (L->state_stride < n_nodes * S) return fail(c, MPLX_ERR_ARG, "%s: the lists' state_stride < n_nodes * node_stride", who);
  if (int rc = usable(t, who)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // yaw pinning: the lists must be final
  if (n_nodes == 0) {
    HIP_TRY(c, hipMemsetAsync(d_next->count, 0, 8, c->stream));
    if (h_count) *h_count = 0;
    return MPLX_OK;
  }
  mplx::TableArgs a = table_args(t);
  a.count = L->count; a.action = L->action; a.cost = L->cost; a.src_hash = L->hash; a.src_state = L->state; a.src_sstride = L->state_stride;
  a.n_rows = n_nodes; a.S = S; a.parent_id = d_parent_id; a.parent_g = d_parent_g; a.g_max = g_max;
  a.entry_id = d_entry_id;
  uint64_t *keys = nullptr;
  if (int rc = run_passes(t, &a, d_next, 0, nullptr, t->time_keys ? &keys : nullptr)) return rc;
  if (keys) {  // the entry's own t row
    HIP_TRY(c, mplx::launch_table_time_keys(L->count, S, n_nodes * S, L->hash, L->state + (int64_t)(t->F - 1) * L->state_stride, keys, c->stream));
    a.src_hash = keys;
  }
  HIP_TRY(c, mplx::launch_table_relax(a, c->stream));
  return h_count ? read_count(t, d_next, h_count) : MPLX_OK;
}

static int seed_table(mplx_table *t, const char *who, const double *h_states, int64_t n, int64_t stride, const double *h_g,
                      const int32_t *h_query, const mplx_table_frontier *d_frontier, int64_t *h_count) {
  mplx_ctx *c = t->c;
  if (n < 0 || n > kMaxEntries || stride < n || (n > 0 && !h_states)) return fail(c, MPLX_ERR_ARG, "%s: need states and 0 <= n <= stride", who);
  if (int rc = check_frontier(c, who, d_frontier)) return rc;
  if (!c->has_params) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_params has not been called", who);
  if (!c->has_U) return fail(c, MPLX_ERR_STATE, "%s: mplx_set_controls has not been called", who);
  if (int rc = usable(t, who)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  if (n == 0) {
    HIP_TRY(c, hipMemsetAsync(d_frontier->count, 0, 8, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_count) *h_count = 0;
    return MPLX_OK;
  }
  const bool multi = t->Q > 1;  // (one query: every seed is query 0 and no kernel looks a query up)
  StageRows s;  // (no output row: read_count below is the call's read-back and synchronise)
  const auto i_st = s.in_rows(h_states, (size_t)stride * 8, (size_t)n * 8, (size_t)t->F), i_g = s.in(h_g, (size_t)n * 8),
             i_q = s.in(multi ? h_query : nullptr, (size_t)n * 4);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx::TableArgs a = table_args(t);
  a.src_query = s.dev<int32_t>(i_q);
  a.src_state = s.dev<double>(i_st); a.src_sstride = n;
  a.n_rows = n; a.S = 1; a.parent_g = s.dev<double>(i_g); a.g_max = INFINITY;
  void *hashes = nullptr;
  if (int rc = run_passes(t, &a, d_frontier, (size_t)n * 8, &hashes)) return rc;
  a.src_hash = (const uint64_t *)hashes;
  HIP_TRY(c, mplx::launch_table_hash(c->dim, c->prm.control, a.src_state, n, n, (uint64_t *)hashes, c->stream));
  if (t->time_keys)  // in place: every entry reads its own hash
    HIP_TRY(c, mplx::launch_table_time_keys(nullptr, 1, n, (const uint64_t *)hashes, a.src_state + (int64_t)(t->F - 1) * n, (uint64_t *)hashes, c->stream));
  HIP_TRY(c, mplx::launch_table_relax(a, c->stream));
  int64_t count = 0;
  if (int rc = read_count(t, d_frontier, &count)) return rc;  // (the arena is free again: the stream is idle)
  if (h_count) *h_count = count;
  return MPLX_OK;
}

int mplx_table_seed(mplx_table *t, const double *h_states, int64_t n, int64_t stride, const double *h_g, const mplx_table_frontier *d_frontier,
                    int64_t *h_count) {
  if (!t) return MPLX_ERR_ARG;
  if (int rc = single_only(t, "mplx_table_seed")) return rc;
  return seed_table(t, "mplx_table_seed", h_states, n, stride, h_g, nullptr, d_frontier, h_count);
}

int mplx_table_seed_multi(mplx_table *t, const double *h_states, int64_t n, int64_t stride, const double *h_g, const int32_t *h_query,
                          const mplx_table_frontier *d_frontier, int64_t *h_count) {
  if (!t) return MPLX_ERR_ARG;
  const char *who = "mplx_table_seed_multi";
  if (n > 0 && !h_query) return fail(t->c, MPLX_ERR_ARG, "%s: NULL h_query", who);
  for (int64_t i = 0; i < n; i++)
    if (h_query[i] < 0 || h_query[i] >= t->Q)
      return fail(t->c, MPLX_ERR_ARG, "%s: h_query[%lld] = %d is not in [0, %d)", who, (long long)i, (int)h_query[i], (int)t->Q);
  return seed_table(t, who, h_states, n, stride, h_g, h_query, d_frontier, h_count);
}

// d_query / h_query null: the plain calls (a table of one query)
static int find_device(mplx_table *t, const char *who, const uint64_t *d_hash, const int32_t *d_query, int64_t n, int32_t *d_id) {
  mplx_ctx *c = t->c;
  if (n < 0 || (n > 0 && (!d_hash || !d_id))) return fail(c, MPLX_ERR_ARG, "%s: NULL argument or n < 0", who);
  if (int rc = usable(t, who)) return rc;
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, mplx::launch_table_find(table_args(t), d_hash, d_query, n, d_id, c->stream));
  return MPLX_OK;
}

static int find_host(mplx_table *t, const char *who, const uint64_t *h_hash, const int32_t *h_query, int64_t n, int32_t *h_id) {
  mplx_ctx *c = t->c;
  if (n < 0 || (n > 0 && (!h_hash || !h_id))) return fail(c, MPLX_ERR_ARG, "%s: NULL argument or n < 0", who);
  if (int rc = usable(t, who)) return rc;
  if (n == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  StageRows s;
  const auto i_h = s.in(h_hash, (size_t)n * 8), o_id = s.out(h_id, (size_t)n * 4), i_q = s.in(h_query, (size_t)n * 4);
  if (int rc = stage_commit(c, &s)) return rc;
  HIP_TRY(c, mplx::launch_table_find(table_args(t), s.dev<uint64_t>(i_h), s.dev<int32_t>(i_q), n, s.dev<int32_t>(o_id), c->stream));
  if (int rc = stage_fetch(c, &s)) return rc;
  observe(t);
  return MPLX_OK;
}

int mplx_table_find_device(mplx_table *t, const uint64_t *d_hash, int64_t n, int32_t *d_id) {
  if (!t) return MPLX_ERR_ARG;
  if (int rc = single_only(t, "mplx_table_find_device")) return rc;
  return find_device(t, "mplx_table_find_device", d_hash, nullptr, n, d_id);
}

int mplx_table_find(mplx_table *t, const uint64_t *h_hash, int64_t n, int32_t *h_id) {
  if (!t) return MPLX_ERR_ARG;
  if (int rc = single_only(t, "mplx_table_find")) return rc;
  return find_host(t, "mplx_table_find", h_hash, nullptr, n, h_id);
}

int mplx_table_find_multi_device(mplx_table *t, const uint64_t *d_hash, const int32_t *d_query, int64_t n, int32_t *d_id) {
  if (!t) return MPLX_ERR_ARG;
  if (n > 0 && !d_query) return fail(t->c, MPLX_ERR_ARG, "mplx_table_find_multi_device: NULL d_query");
  return find_device(t, "mplx_table_find_multi_device", d_hash, d_query, n, d_id);
}

int mplx_table_find_multi(mplx_table *t, const uint64_t *h_hash, const int32_t *h_query, int64_t n, int32_t *h_id) {
  if (!t) return MPLX_ERR_ARG;
  const char *who = "mplx_table_find_multi";
  if (n > 0 && !h_query) return fail(t->c, MPLX_ERR_ARG, "%s: NULL h_query", who);
  for (int64_t i = 0; i < n; i++)
    if (h_query[i] < 0 || h_query[i] >= t->Q)
      return fail(t->c, MPLX_ERR_ARG, "%s: h_query[%lld] = %d is not in [0, %d)", who, (long long)i, (int)h_query[i], (int)t->Q);
  return find_host(t, who, h_hash, h_query, n, h_id);
}

int mplx_table_path(mplx_table *t, int32_t id, int32_t *h_ids, int32_t *h_actions, int64_t cap, int64_t *n_edges) {
  if (!t) return MPLX_ERR_ARG;
  mplx_ctx *c = t->c;
  const char *who = "mplx_table_path";
  if (!h_ids || !n_edges || cap < 0 || cap > kMaxEntries || (cap > 0 && !h_actions)) return fail(c, MPLX_ERR_ARG, "%s: NULL argument or cap < 0", who);
  if (int rc = usable(t, who)) return rc;
  MPLX_GUARD_BEGIN
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  StageLayout l;
  const size_t o_ids = l.add((size_t)(cap + 1) * 4), o_act = l.add((size_t)cap * 4), o_len = l.add(8);
  if (int rc = stage_commit(c, &l)) return rc;
  HIP_TRY(c, mplx::launch_table_path(table_args(t), id, (int32_t *)(l.base + o_ids), (int32_t *)(l.base + o_act), cap, (int64_t *)(l.base + o_len), c->stream));
  int64_t len = 0;
  HIP_TRY(c, stage_out(c, &len, l.base + o_len, 8));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  observe(t);
  if (len == -1) return fail(c, MPLX_ERR_ARG, "%s: the chain of node %d has more than cap = %lld edges", who, id, (long long)cap);
  if (len == -2) return fail(c, MPLX_ERR_ARG, "%s: node %d is not in the table", who, id);
  if (len < 0) return fail(c, MPLX_ERR_STATE, "%s: no seed within n_nodes steps of node %d", who, id);
  std::vector<int32_t> ids((size_t)len + 1), act((size_t)len);
  HIP_TRY(c, stage_out(c, ids.data(), l.base + o_ids, ids.size() * 4));
  if (len > 0) HIP_TRY(c, stage_out(c, act.data(), l.base + o_act, act.size() * 4));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::reverse_copy(ids.begin(), ids.end(), h_ids);   // the walk is leaf first
  std::reverse_copy(act.begin(), act.end(), h_actions);
  *n_edges = len;
  return MPLX_OK;
  MPLX_GUARD_END(c)
}

}  // extern "C"
