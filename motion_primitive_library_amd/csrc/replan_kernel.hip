// replan_kernel.hip -- re-rooting and repair of the node table of table_kernel.hip after a map edit
// (include/mplx_replan.h): which nodes still hang, edge by valid edge, below the new root, and the frontier of them.
//
// The table's discipline holds: a launch boundary is the only ordering between passes, no
// workgroup waits for another, only order-free integer atomics (add, or) decide anything, and ranks come from prefix
// sums in id order -- every output is a pure function of the inputs.
//
// One rebase is 6 + P launches:
//   edge     (check_edges) one lane per node: gathers state[pred], evaluates the ONE pair (state[pred], U[pred_action])
//            with the functions of mplx_pair_device.h -- the step of rollout_kernel.hip -- and writes one byte bad[id]
//   init     one lane per node: root -> KEEP; no predecessor, or a bad edge -> DROP; otherwise UNKNOWN with jump = pred.
//            Roots and bad edges are counted by ballot, one atomicAdd per wave
//   resolve  P = ceil(log2(bound of n_nodes)) + 1 passes of pointer doubling.  A pass reads buffer A and writes buffer B:
//            an UNKNOWN node whose jump target is decided adopts the decision, otherwise it takes the target's jump.
//            An UNKNOWN node keeps, between passes, the ancestor min(2^k, d) edges up, d = its distance to the nearest
//            ancestor decided by init: a chain of d <= n - 1 edges is decided after ceil(log2 d) + 1 passes, and what is
//            UNKNOWN after P passes lies on a cycle and is dropped.  pred[id] < id is NOT assumed.
//   apply    per tile of 4096 ids: dropped nodes back to g = +inf, pred = pred_action = -1; kept roots lose their
//            back-pointer; kept nodes marked and counted per tile (and, one atomicAdd per tile, in all)
//   scan     table_kernel.hip's second scan: prefix sums of the tile counts, the frontier count or FRONTIER_FULL
//   emit     kept nodes in id order -> id, g and the state rows gathered from the table
// Every index is checked where it is formed: ids and predecessors against the table's own node count, rows against the
// frontier's capacity, actions against the control table.  A table with a status bit makes every pass return at its
// first instruction.
#include "mplx_internal.h"
#include "mplx_pair_device.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kBlock = 256;
constexpr int kItems = kTableTile / kBlock;
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;
constexpr uint8_t kUnknown = 0, kKeep = 1, kDrop = 2;

__device__ __forceinline__ int64_t node_count(const ReplanArgs &R) {
  const int64_t n = R.ctl->n_nodes;
  return n < 0 ? 0 : (n < R.cap ? n : R.cap);
}

// root(id) of include/mplx_replan.h; id < n
__device__ __forceinline__ bool is_root(const ReplanArgs &R, int64_t id) {
  if (!__builtin_isfinite(__longlong_as_double((long long)R.g[id]))) return false;
  int32_t r = R.root_id;
  if (R.root_of_query) {
    int32_t q = R.query ? R.query[id] : 0;
    if (q < 0 || q >= R.n_queries) return false;  // (never: the column holds only queries)
    r = R.root_of_query[q];
  }
  return r >= 0 ? id == (int64_t)r : R.pred[id] == -1;
}

template <int D, int K, bool YAW>
__global__ __launch_bounds__(kBlock) void replan_edge_kernel(const ReplanArgs R) {
  if (R.ctl->status) return;
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = node_count(R);
  if (id >= n) return;
  const ExpandArgs &A = R.env;
  uint8_t bad = 0;
  const int32_t p = R.pred[id];
  if (p >= 0 && !is_root(R, id)) {
    const int32_t a = R.pred_action[id];
    if (p >= n || a < 0 || a >= A.nU) {
      bad = 1;  // (the control table and the node arrays are never read out of range)
    } else {
      const double *up = A.U + (int64_t)a * A.udim;
      double u[D], uy = 0.0;
#pragma unroll
      for (int i = 0; i < D; i++) u[i] = up[i];
      if (YAW) uy = up[D];
      pair::Pair<D, K, YAW> P;
#pragma unroll
      for (int i = 0; i < D; i++) {
        // (rows the control order does not read: 0.0, as the dense kernel loads them)
        P.cpos[i] = R.state[(int64_t)(0 * D + i) * R.cap + p];
        P.cvel[i] = (K >= 2) ? R.state[(int64_t)(1 * D + i) * R.cap + p] : 0.0;
        P.cacc[i] = (K >= 3) ? R.state[(int64_t)(2 * D + i) * R.cap + p] : 0.0;
        P.cjrk[i] = (K >= 4) ? R.state[(int64_t)(3 * D + i) * R.cap + p] : 0.0;
      }
      P.cyaw = YAW ? R.state[(int64_t)(4 * D) * R.cap + p] : 0.0;
      P.init(u, uy, A.dt);
      bool valid = true, amb = false;
      if (YAW && A.yaw_max > 0) valid = P.heading_valid(nullptr, 0, cos(A.yaw_max), A.yaw.margin, A.yaw.tie_yaw, &amb);
      valid = P.limits_valid(A, valid);
      uint8_t st;
      double cost;
      int iters;
      P.classify(A, valid, &st, &cost, &iters);
      if (st != 1 || P.h_next != R.hash[id] || (amb && R.band)) {
        bad = 1;
      } else {
        const double cand = __longlong_as_double((long long)R.g[p]) + cost;
        bad = cand > __longlong_as_double((long long)R.g[id]) ? 1 : 0;
      }
    }
  }
  R.bad[id] = bad;
}

__global__ __launch_bounds__(kBlock) void replan_init_kernel(const ReplanArgs R) {
  if (R.ctl->status) return;  // (uniform)
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = node_count(R);
  bool root = false, bad_edge = false;
  if (id < n) {
    root = is_root(R, id);
    const int32_t p = R.pred[id];
    uint8_t d = kKeep;
    if (!root) {
      bad_edge = p >= 0 && (p >= n || (R.check_edges && R.bad[id] != 0));
      d = (p < 0 || bad_edge) ? kDrop : kUnknown;
    }
    R.dec[0][id] = d;
    R.jump[0][id] = d == kUnknown ? p : -1;
  }
  const unsigned long long br = __ballot(root), bb = __ballot(bad_edge);
  if ((threadIdx.x & 63) != 0) return;
  if (br) atomicAdd((unsigned long long *)&R.counters->n_roots, (unsigned long long)__popcll(br));
  if (bb) atomicAdd((unsigned long long *)&R.counters->n_bad_edges, (unsigned long long)__popcll(bb));
}

// reads buffers `from`, writes buffers 1 - from: no result depends on which lane ran first
__global__ __launch_bounds__(kBlock) void replan_resolve_kernel(const ReplanArgs R, int from) {
  if (R.ctl->status) return;
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x, n = node_count(R);
  if (id >= n) return;
  const uint8_t *dA = R.dec[from];
  const int32_t *jA = R.jump[from];
  uint8_t d = dA[id];
  int32_t j = jA[id];
  if (d == kUnknown) {
    if (j < 0 || j >= n) {
      d = kDrop;  // (never: an UNKNOWN node's jump is a node)
    } else {
      const uint8_t dj = dA[j];
      if (dj != kUnknown) d = dj;
      else j = jA[j];
    }
  }
  R.dec[1 - from][id] = d;
  R.jump[1 - from][id] = j;
}

__global__ __launch_bounds__(kBlock) void replan_apply_kernel(const ReplanArgs R, int last) {
  if (R.ctl->status) return;  // (uniform: nothing below is skipped by part of a workgroup)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = node_count(R), base = (int64_t)blockIdx.x * kTableTile;
  const uint8_t *dec = R.dec[last];
  uint32_t cnt = 0;
  for (int i = 0; i < kItems; i++) {
    const int64_t id = base + (int64_t)i * kBlock + threadIdx.x;
    bool m = false;
    if (id < n) {
      m = dec[id] == kKeep;
      if (!m) {
        R.g[id] = kInfBits;
        R.pred[id] = -1;
        R.pred_action[id] = -1;
      } else if (R.jump[last][id] < 0) {  // decided by the init pass as KEEP: a root
        R.pred[id] = -1;
        R.pred_action[id] = -1;
      }
      R.mark[id] = m ? 1 : 0;
    }
    cnt += (uint32_t)__popcll(__ballot(m));  // the wave's count, in every lane
  }
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kBlock / 64; w++) t += wsum[w];
    R.tot[blockIdx.x] = t;
    if (t) atomicAdd((unsigned long long *)&R.counters->n_kept, (unsigned long long)t);
  }
}

// Rank of every kept node of a tile in id order = its frontier row (open_kernel.hip's emit pass, without the flags).
__global__ __launch_bounds__(kBlock) void replan_emit_kernel(const ReplanArgs R) {
  if (R.ctl->emit == 0) return;  // (uniform; the scan sets it only when the call met no status bit)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = node_count(R), base = (int64_t)blockIdx.x * kTableTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t run = R.tot[blockIdx.x];
  for (int i = 0; i < kItems; i++) {
    const int64_t id = base + (int64_t)i * kBlock + threadIdx.x;
    const bool m = id < n && R.mark[id] != 0;
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
    if (!m || r >= R.f_cap) continue;
    R.f_id[r] = (int32_t)id;
    R.f_g[r] = __longlong_as_double((long long)R.g[id]);
    for (int f = 0; f < R.n_fields; f++) R.f_state[(int64_t)f * R.f_stride + r] = R.state[(int64_t)f * R.cap + id];
  }
}

template <int D>
hipError_t edge_dim(int control, const ReplanArgs &a, dim3 grid, hipStream_t s) {
  const dim3 block(kBlock);
  switch (control) {
    case 0x01: hipLaunchKernelGGL((replan_edge_kernel<D, 1, false>), grid, block, 0, s, a); break;
    case 0x03: hipLaunchKernelGGL((replan_edge_kernel<D, 2, false>), grid, block, 0, s, a); break;
    case 0x07: hipLaunchKernelGGL((replan_edge_kernel<D, 3, false>), grid, block, 0, s, a); break;
    case 0x0f: hipLaunchKernelGGL((replan_edge_kernel<D, 4, false>), grid, block, 0, s, a); break;
    case 0x11: hipLaunchKernelGGL((replan_edge_kernel<D, 1, true>), grid, block, 0, s, a); break;
    case 0x13: hipLaunchKernelGGL((replan_edge_kernel<D, 2, true>), grid, block, 0, s, a); break;
    case 0x17: hipLaunchKernelGGL((replan_edge_kernel<D, 3, true>), grid, block, 0, s, a); break;
    case 0x1f: hipLaunchKernelGGL((replan_edge_kernel<D, 4, true>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_replan_rebase(int dim, int control, const ReplanArgs &a, int passes, hipStream_t s) {
  const int64_t n = a.n_bound > 0 ? a.n_bound : 1;
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), per_tile((unsigned)a.n_tiles), block(kBlock);
  if (hipError_t e = hipMemsetAsync(a.counters, 0, sizeof(ReplanResult), s)) return e;
  if (a.check_edges) {
    hipError_t e = dim == 2 ? edge_dim<2>(control, a, per_node, s) : dim == 3 ? edge_dim<3>(control, a, per_node, s) : hipErrorInvalidValue;
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(replan_init_kernel, per_node, block, 0, s, a);
  for (int k = 0; k < passes; k++) hipLaunchKernelGGL(replan_resolve_kernel, per_node, block, 0, s, a, k & 1);
  hipLaunchKernelGGL(replan_apply_kernel, per_tile, block, 0, s, a, passes & 1);
  if (hipError_t e = hipGetLastError()) return e;
  TableArgs t{};
  t.ctl = a.ctl;
  t.mirror = a.mirror;
  t.tot = a.tot;
  t.n_tiles = a.n_tiles;
  t.f_cap = a.f_cap;
  t.f_count = a.f_count;
  if (hipError_t e = launch_table_scan_frontier(t, s)) return e;
  hipLaunchKernelGGL(replan_emit_kernel, per_tile, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
