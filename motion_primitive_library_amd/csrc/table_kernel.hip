// table_kernel.hip -- the persistent node table of include/mplx_table.h: what GraphSearch::Astar does with the
// successors of an expanded node (reference include/mpl_planner/common/graph_search.h:79-143: find or create the child
// in StateSpace::hm_, tentative = g + cost, keep it if smaller), for whole batches of successor lists where the
// expansion kernels left them in HBM, plus the next frontier.
//
// The table is open addressing in HBM keyed by the 64-bit lattice hash, as in post_kernel.hip: linear probing from a
// mixed hash, 64-bit CAS for the key, key and id in one 16-byte slot, a dedicated slot for the one hash equal to the
// empty marker.  Unlike that one-call table it persists, and its probe loop is bounded by the table's length.
// A table with several queries (include/mplx_multi.h) keeps one such region of slots, and one dedicated slot, per
// query: claim and find add the region's base, the number pass writes the new node's query, nothing else changes.
//
// One relax call is nine launches; a launch boundary is the only ordering between passes (no grid-wide barrier, no
// spinning workgroup: DESIGN.md 11.1), and inside a pass only order-free atomics decide anything:
//   claim    per counting entry: find or insert the key; keys new in this call: atomicMin(first_e, e)
//   mark     entries with first_e == e (one per new key), counted per tile of 4096 entries
//   scan     exclusive prefix sums of the tile counts (one workgroup); n_nodes advances, or NODES_FULL
//   number   ids = nodes before the call + rank in entry order; the new nodes' rows, their state columns
//   lower    atomicMin of cand's bit pattern on g; an entry that lowered g stamps the node with the call's tag
//   pick     entries of stamped nodes with cand == g: atomicMin of (tag, e) -- the smallest such e wins
//   mark     the winners, which write pred / pred_action; counted per tile
//   scan     ... the frontier count, or FRONTIER_FULL; the control block goes to its pinned mirror
//   emit     winners in entry order -> id, g and the state rows gathered from the table
// Every array index is checked where it is formed: a full table, a full node array or a short frontier set a status
// bit and drop the write.  Once a bit is set every later pass (and call) returns at its first instruction.
// Traffic per counting entry: DESIGN.md 4.10.
#include "mplx_internal.h"
#include "mplx_pair_device.h"  // lattice_hash of a seed state

namespace mplx {
namespace {

constexpr uint64_t kEmpty = ~0ull;
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kBlock = 256;
constexpr int kItems = kTableTile / kBlock;
constexpr uint32_t kNodesFull = 1, kProbeFull = 2, kFrontierFull = 4;  // MPLX_TABLE_* of include/mplx_table.h

__device__ __forceinline__ uint64_t mix(uint64_t h) {  // table position only; never leaves the device
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdULL;
  h ^= h >> 33;
  return h;
}

// Does entry e count (include/mplx_table.h), and with which candidate?  Reads nothing of an entry past count[k].
// n_before: the nodes the table held before the call -- on a table with several queries a parent must be one of them
// (its query is the entry's).
__device__ __forceinline__ bool entry(const TableArgs &A, int64_t e, int64_t n_before, int64_t *row, double *cand_out) {
  const int64_t k = e / A.S;
  if (A.count && (int)(e - k * A.S) >= A.count[k]) return false;
  if (A.parent_id && A.parent_id[k] < 0) return false;
  if (A.query && A.parent_id && A.parent_id[k] >= n_before) return false;
  double cand = A.parent_g ? A.parent_g[k] : 0.0;
  if (A.cost) {
    const double c = A.cost[e];
    if (!__builtin_isfinite(c)) return false;  // blocked successors: graph_search.h:81
    cand = cand + c;                           // graph_search.h:107
  }
  if (!(__builtin_isfinite(cand) && cand >= 0.0 && cand <= A.g_max)) return false;
  *row = k;
  *cand_out = cand + 0.0;  // -0.0 -> +0.0: the bit patterns of the candidates order like the candidates
  return true;
}

// The query of a counting entry of a table with several queries: the seed's own, or its parent's (an id below n_before).
__device__ __forceinline__ int32_t entry_query(const TableArgs &A, int64_t e, int64_t row) {
  return A.src_query ? A.src_query[e] : A.query[A.parent_id[row]];
}

__global__ __launch_bounds__(kBlock) void table_claim_kernel(const TableArgs A) {
  if (A.ctl->status) return;
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= A.n_rows * A.S) return;
  int64_t k;
  double cand;
  uint32_t s = kNone;
  if (entry(A, e, A.query ? A.ctl->n_nodes : 0, &k, &cand)) {
    const uint64_t h = A.src_hash[e];
    // a query's keys live in its own region of q_slots slots: the compare stays the hash alone
    uint64_t q = 0;
    if (A.query) {
      const int32_t qq = entry_query(A, e, k);
      q = (qq >= 0 && qq < A.n_queries) ? (uint64_t)qq : 0;  // (the host checks the seeds; the column holds only queries)
    }
    if (h == kEmpty) {
      s = (uint32_t)(A.n_slots + q);  // the one hash the key field cannot hold
    } else {
      const uint64_t mask = A.q_slots - 1, base = q * A.q_slots;
      uint64_t p = mix(h) & mask;
      for (uint64_t tries = 0; tries < A.q_slots; tries++) {
        TableSlot *sl = &A.slots[base + p];
        uint64_t key = sl->key;  // (a stale "empty" only costs the CAS; a key never changes once it is set)
        if (key == kEmpty) key = atomicCAS((unsigned long long *)&sl->key, (unsigned long long)kEmpty, (unsigned long long)h);
        if (key == kEmpty || key == h) {
          s = (uint32_t)(base + p);
          break;
        }
        p = (p + 1) & mask;
      }
      // every slot of the region holds another key.  One query: more keys than slots, hence than node_capacity
      // (< n_slots); several: the query's region is full -- both bits either way
      if (s == kNone) atomicOr(&A.ctl->status, kProbeFull | kNodesFull);
    }
    // a key without an id is new in this call (ids are written by the number pass, behind a launch boundary)
    if (s != kNone && A.slots[s].id < 0) atomicMin(&A.slots[s].first_e, (uint32_t)e);
  }
  A.ent[e] = s;
}

// Marks of a tile pass.  MODE 0: the first entry of every new key.  MODE 1: the winning entry of every improved node,
// which writes the node's back-pointer.
template <int MODE>
__device__ __forceinline__ bool is_marked(const TableArgs &A, int64_t e) {
  const uint32_t v = A.ent[e];
  if (MODE == 0) {
    if (v == kNone) return false;
    const TableSlot sl = A.slots[v];
    return sl.id < 0 && sl.first_e == (uint32_t)e;
  }
  const int32_t id = (int32_t)v;
  if (id < 0) return false;
  if (A.pick[id] != (((unsigned long long)A.tag << 32) | (unsigned long long)e)) return false;
  A.pred[id] = A.parent_id ? A.parent_id[e / A.S] : -1;
  A.pred_action[id] = A.action ? A.action[e] : -1;
  return true;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void table_mark_kernel(const TableArgs A) {
  if (A.ctl->status) return;  // (uniform: nothing below is skipped by part of a workgroup)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = A.n_rows * A.S, base = (int64_t)blockIdx.x * kTableTile;
  uint32_t cnt = 0;
  for (int i = 0; i < kItems; i++) {
    const int64_t e = base + (int64_t)i * kBlock + threadIdx.x;
    bool m = false;
    if (e < n) {
      m = is_marked<MODE>(A, e);
      A.mark[e] = m ? 1 : 0;
    }
    cnt += (uint32_t)__popcll(__ballot(m));  // the wave's count, in every lane
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kBlock / 64; w++) t += wsum[w];
    A.tot[blockIdx.x] = t;
  }
}

// Exclusive prefix sums of the tile counts, in place, by one workgroup (n_tiles <= 2^19: each thread sums a contiguous
// slice, the slice sums are scanned through LDS -- pack_kernel.hip's scan), then what the total decides.
template <int MODE>
__global__ __launch_bounds__(1024) void table_scan_kernel(const TableArgs A) {
  __shared__ uint32_t part[1024];
  const uint32_t status = A.ctl->status;
  const int t = threadIdx.x;
  uint32_t total = 0;
  if (status == 0) {
    const int64_t per = (A.n_tiles + 1023) / 1024;
    const int64_t a = (int64_t)t * per < A.n_tiles ? (int64_t)t * per : A.n_tiles, b = a + per < A.n_tiles ? a + per : A.n_tiles;
    uint32_t s = 0;
    for (int64_t k = a; k < b; k++) s += A.tot[k];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const uint32_t v = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += v;
      __syncthreads();
    }
    uint32_t run = part[t] - s;
    for (int64_t k = a; k < b; k++) {
      const uint32_t c = A.tot[k];
      A.tot[k] = run;
      run += c;
    }
    total = part[1023];
  }
  __syncthreads();  // every thread has read the status before thread 0 may change it
  if (t != 0) return;
  if (MODE == 0) {
    if (status) return;
    const int64_t base = A.ctl->n_nodes;
    A.ctl->base = (int32_t)base;
    if (base + (int64_t)total > A.cap) atomicOr(&A.ctl->status, kNodesFull);
    else A.ctl->n_nodes = (int32_t)(base + (int64_t)total);
  } else {
    int64_t cnt = 0;
    if (status == 0) {
      cnt = total;
      if (cnt > A.f_cap) {
        atomicOr(&A.ctl->status, kFrontierFull);
        cnt = A.f_cap;
      }
    }
    A.ctl->emit = status == 0 ? 1 : 0;
    *A.f_count = cnt;
    // the pinned mirror: what the host reads, without a copy, once it has waited for the stream
    __hip_atomic_store(&A.mirror->n_nodes, (int64_t)A.ctl->n_nodes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&A.mirror->status, __hip_atomic_load(&A.ctl->status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Rank of every marked entry of a tile in entry order, and what the rank is for.  MODE 0: the new node.  MODE 1: the
// frontier row.
template <int MODE>
__global__ __launch_bounds__(kBlock) void table_apply_kernel(const TableArgs A) {
  if (MODE == 0 ? A.ctl->status != 0 : A.ctl->emit == 0) return;  // (uniform)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = A.n_rows * A.S, base = (int64_t)blockIdx.x * kTableTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t run = A.tot[blockIdx.x];
  const int64_t base_id = A.ctl->base;
  for (int i = 0; i < kItems; i++) {
    const int64_t e = base + (int64_t)i * kBlock + threadIdx.x;
    const bool m = e < n && A.mark[e] != 0;
    const unsigned long long bal = __ballot(m);
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int w = 0; w < kBlock / 64; w++) {
      if (w < wave) before += wsum[w];
      all += wsum[w];
    }
    __syncthreads();
    const int64_t r = run + before + (int64_t)__popcll(bal & ((1ull << lane) - 1ull));
    run += all;
    if (!m) continue;
    if (MODE == 0) {
      const int64_t id = base_id + r;
      if (id >= A.cap) continue;  // (the scan has set NODES_FULL in that case: never taken)
      A.slots[A.ent[e]].id = (int32_t)id;
      A.hash[id] = A.src_hash[e];
      A.g[id] = 0x7ff0000000000000ull;  // +inf
      A.pick[id] = ~0ull;
      A.pred[id] = -1;
      A.pred_action[id] = -1;
      if (A.query) A.query[id] = entry_query(A, e, e / A.S);  // (a counting entry: its parent is an older node)
      for (int f = 0; f < A.n_fields; f++) A.state[(int64_t)f * A.cap + id] = A.src_state[(int64_t)f * A.src_sstride + e];
    } else {
      if (r >= A.f_cap) continue;
      const int32_t id = (int32_t)A.ent[e];
      A.f_id[r] = id;
      A.f_g[r] = __longlong_as_double((long long)A.g[id]);
      for (int f = 0; f < A.n_fields; f++) A.f_state[(int64_t)f * A.f_stride + r] = A.state[(int64_t)f * A.cap + id];
    }
  }
}

__global__ __launch_bounds__(kBlock) void table_lower_kernel(const TableArgs A) {
  if (A.ctl->status) return;
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= A.n_rows * A.S) return;
  const uint32_t s = A.ent[e];
  int32_t id = -1;
  if (s != kNone) {
    id = A.slots[s].id;
    int64_t k;
    double cand;
    if (id >= 0 && id < A.cap && entry(A, e, A.query ? A.ctl->base : 0, &k, &cand)) {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(cand);
      const unsigned long long old = atomicMin(&A.g[id], bits);
      if (old > bits) atomicMin(&A.pick[id], ((unsigned long long)A.tag << 32) | 0xffffffffull);  // improved in this call
    } else {
      id = -1;
    }
  }
  A.ent[e] = (uint32_t)id;
  if (A.entry_id) A.entry_id[e] = id;
}

__global__ __launch_bounds__(kBlock) void table_pick_kernel(const TableArgs A) {
  if (A.ctl->status) return;
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= A.n_rows * A.S) return;
  const int32_t id = (int32_t)A.ent[e];
  if (id < 0) return;
  if ((uint32_t)(A.pick[id] >> 32) != A.tag) return;  // not improved in this call
  int64_t k;
  double cand;
  if (!entry(A, e, A.query ? A.ctl->base : 0, &k, &cand)) return;
  if ((unsigned long long)__double_as_longlong(cand) == A.g[id]) atomicMin(&A.pick[id], ((unsigned long long)A.tag << 32) | (unsigned long long)e);
}

__global__ void table_clear_kernel(const TableArgs A) {
  A.ctl->n_nodes = 0;
  A.ctl->base = 0;
  A.ctl->status = 0;
  A.ctl->emit = 0;
  __hip_atomic_store(&A.mirror->n_nodes, (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&A.mirror->status, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int D, int K, bool YAW>
__global__ __launch_bounds__(kBlock) void table_hash_kernel(const double *states, int64_t n, int64_t stride, uint64_t *hash) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  double s[4 * D + 1];
#pragma unroll
  for (int f = 0; f < 4 * D + 1; f++) s[f] = states[(int64_t)f * stride + k];
  hash[k] = pair::lattice_hash<D, K, YAW>(s, s + D, s + 2 * D, s + 3 * D, s[4 * D]);
}

// Time keys (mplx_table_set_time_keys): the last hash_combine of Waypoint::enable_t (waypoint.h:119-122)
__global__ __launch_bounds__(kBlock) void table_time_key_kernel(const int32_t *count, int64_t S, int64_t n, const uint64_t *hash,
                                                                const double *t, uint64_t *key) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n) return;
  if (count) {
    const int64_t k = e / S;
    if ((int)(e - k * S) >= count[k]) return;  // nothing of an entry past count[k] is read
  }
  uint64_t h = hash[e];
  dev::fold(h, pair::quantise(t[e], 0.1));
  key[e] = h;
}

template <int D>
hipError_t hash_dim(int control, const double *states, int64_t n, int64_t stride, uint64_t *hash, hipStream_t s) {
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  switch (control) {
    case 0x01: hipLaunchKernelGGL((table_hash_kernel<D, 1, false>), grid, block, 0, s, states, n, stride, hash); break;
    case 0x03: hipLaunchKernelGGL((table_hash_kernel<D, 2, false>), grid, block, 0, s, states, n, stride, hash); break;
    case 0x07: hipLaunchKernelGGL((table_hash_kernel<D, 3, false>), grid, block, 0, s, states, n, stride, hash); break;
    case 0x0f: hipLaunchKernelGGL((table_hash_kernel<D, 4, false>), grid, block, 0, s, states, n, stride, hash); break;
    case 0x11: hipLaunchKernelGGL((table_hash_kernel<D, 1, true>), grid, block, 0, s, states, n, stride, hash); break;
    case 0x13: hipLaunchKernelGGL((table_hash_kernel<D, 2, true>), grid, block, 0, s, states, n, stride, hash); break;
    case 0x17: hipLaunchKernelGGL((table_hash_kernel<D, 3, true>), grid, block, 0, s, states, n, stride, hash); break;
    case 0x1f: hipLaunchKernelGGL((table_hash_kernel<D, 4, true>), grid, block, 0, s, states, n, stride, hash); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

__global__ __launch_bounds__(kBlock) void table_find_kernel(const TableArgs A, const uint64_t *hash, const int32_t *query, int64_t n,
                                                            int32_t *id) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t h = hash[i];
  const int64_t q = query ? (int64_t)query[i] : 0;
  int32_t out = -1;
  if (q < 0 || q >= A.n_queries) {
    // no such query: not in the table
  } else if (h == kEmpty) {
    out = A.slots[A.n_slots + (uint64_t)q].id;
  } else {
    const uint64_t mask = A.q_slots - 1, base = (uint64_t)q * A.q_slots;
    uint64_t p = mix(h) & mask;
    for (uint64_t tries = 0; tries < A.q_slots; tries++) {
      const uint64_t key = A.slots[base + p].key;
      if (key == h) out = A.slots[base + p].id;
      if (key == h || key == kEmpty) break;
      p = (p + 1) & mask;
    }
  }
  id[i] = out < 0 ? -1 : out;
}

__global__ void table_path_kernel(const TableArgs A, int32_t id, int32_t *ids, int32_t *actions, int64_t cap, int64_t *len) {
  const int64_t n = A.ctl->n_nodes;
  if (id < 0 || id >= n) {
    *len = -2;
    return;
  }
  int64_t edges = 0;
  int32_t cur = id;
  ids[0] = id;
  for (int64_t step = 0; step < n; step++) {
    const int32_t p = A.pred[cur];
    if (p < 0) {
      *len = edges;
      return;
    }
    if (p >= n) {
      *len = -2;
      return;
    }
    if (edges >= cap) {
      *len = -1;
      return;
    }
    actions[edges] = A.pred_action[cur];
    edges++;
    ids[edges] = p;
    cur = p;
  }
  *len = -3;
}

}  // namespace

hipError_t launch_table_relax(const TableArgs &a, hipStream_t s) {
  const int64_t n = a.n_rows * a.S;
  if (n <= 0) return hipSuccess;
  const dim3 per_entry((unsigned)((n + kBlock - 1) / kBlock)), per_tile((unsigned)a.n_tiles), block(kBlock);
  hipLaunchKernelGGL(table_claim_kernel, per_entry, block, 0, s, a);
  hipLaunchKernelGGL(table_mark_kernel<0>, per_tile, block, 0, s, a);
  hipLaunchKernelGGL(table_scan_kernel<0>, dim3(1), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(table_apply_kernel<0>, per_tile, block, 0, s, a);
  hipLaunchKernelGGL(table_lower_kernel, per_entry, block, 0, s, a);
  hipLaunchKernelGGL(table_pick_kernel, per_entry, block, 0, s, a);
  hipLaunchKernelGGL(table_mark_kernel<1>, per_tile, block, 0, s, a);
  hipLaunchKernelGGL(table_scan_kernel<1>, dim3(1), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(table_apply_kernel<1>, per_tile, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_table_scan_frontier(const TableArgs &a, hipStream_t s) {
  hipLaunchKernelGGL(table_scan_kernel<1>, dim3(1), dim3(1024), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_table_clear(const TableArgs &a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.slots, 0xff, (a.n_slots + (uint64_t)a.n_queries) * sizeof(TableSlot), s)) return e;
  hipLaunchKernelGGL(table_clear_kernel, dim3(1), dim3(1), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_table_hash(int dim, int control, const double *states, int64_t n, int64_t stride, uint64_t *hash, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (dim == 2) return hash_dim<2>(control, states, n, stride, hash, s);
  if (dim == 3) return hash_dim<3>(control, states, n, stride, hash, s);
  return hipErrorInvalidValue;
}

hipError_t launch_table_time_keys(const int32_t *count, int64_t S, int64_t n, const uint64_t *hash, const double *t, uint64_t *key,
                                  hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(table_time_key_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, count, S, n, hash, t, key);
  return hipGetLastError();
}

hipError_t launch_table_find(const TableArgs &a, const uint64_t *hash, const int32_t *query, int64_t n, int32_t *id, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(table_find_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a, hash, query, n, id);
  return hipGetLastError();
}

hipError_t launch_table_path(const TableArgs &a, int32_t id, int32_t *ids, int32_t *actions, int64_t cap, int64_t *len, hipStream_t s) {
  hipLaunchKernelGGL(table_path_kernel, dim3(1), dim3(1), 0, s, a, id, ids, actions, cap, len);
  return hipGetLastError();
}

}  // namespace mplx
