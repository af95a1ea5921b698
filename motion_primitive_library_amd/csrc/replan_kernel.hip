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
// The timed rebase (include/mplx_replan_timed.h) is the same launches with two differences: its edge pass is the TIMED
// instantiation of the edge kernel (the key fold of a table with time keys, the wait rule), and between the edge pass
// and init a reservation pass (replan_reserve_kernel, described where it stands) tests every kept edge against a
// reservation table and sets bad[id] where it conflicts or leaves the horizon.
// Every index is checked where it is formed: ids and predecessors against the table's own node count, rows against the
// frontier's capacity, actions against the control table.  A table with a status bit makes every pass return at its
// first instruction.
#include "mplx_internal.h"
#include "mplx_pair_device.h"
#include "mplx_traj_device.h"

#include <math.h>

#include <type_traits>

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

__device__ __forceinline__ const ReplanArgs &base_of(const ReplanArgs &a) { return a; }
__device__ __forceinline__ const ReplanArgs &base_of(const ReplanTimedArgs &a) { return a.R; }

// TIMED (include/mplx_replan_timed.h): the identity test compares the key the hash column holds -- with time keys
// mplx_time_key(h_next, tp + dt), table_kernel.hip's fold --, and the zero action's dropped successor is a wait edge,
// held by the eligibility and the cost of wait_kernel.hip.  Without TIMED the kernel is the untimed rebase's.
template <int D, int K, bool YAW, bool TIMED>
__global__ __launch_bounds__(kBlock) void replan_edge_kernel(const std::conditional_t<TIMED, ReplanTimedArgs, ReplanArgs> X) {
  const ReplanArgs &R = base_of(X);
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
      uint64_t key = P.h_next;
      bool holds = st == 1 && !(amb && R.band);
      if constexpr (TIMED) {
        if (a == X.a0 && P.h_next == P.h_curr) {  // a wait edge (a0 = -1: there is none)
          holds = X.allow_wait != 0 && P.wait_eligible(valid);
          cost = P.wait_cost(A);
        }
        if (X.time_keys) {
          const double tc = R.state[(int64_t)(4 * D + 1) * R.cap + p] + A.dt;
          dev::fold(key, pair::quantise(tc, 0.1));
        }
      }
      if (!holds || key != R.hash[id]) {
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

template <int D, bool TIMED>
hipError_t edge_dim(int control, const std::conditional_t<TIMED, ReplanTimedArgs, ReplanArgs> &a, dim3 grid, hipStream_t s) {
  const dim3 block(kBlock);
  switch (control) {
    case 0x01: hipLaunchKernelGGL((replan_edge_kernel<D, 1, false, TIMED>), grid, block, 0, s, a); break;
    case 0x03: hipLaunchKernelGGL((replan_edge_kernel<D, 2, false, TIMED>), grid, block, 0, s, a); break;
    case 0x07: hipLaunchKernelGGL((replan_edge_kernel<D, 3, false, TIMED>), grid, block, 0, s, a); break;
    case 0x0f: hipLaunchKernelGGL((replan_edge_kernel<D, 4, false, TIMED>), grid, block, 0, s, a); break;
    case 0x11: hipLaunchKernelGGL((replan_edge_kernel<D, 1, true, TIMED>), grid, block, 0, s, a); break;
    case 0x13: hipLaunchKernelGGL((replan_edge_kernel<D, 2, true, TIMED>), grid, block, 0, s, a); break;
    case 0x17: hipLaunchKernelGGL((replan_edge_kernel<D, 3, true, TIMED>), grid, block, 0, s, a); break;
    case 0x1f: hipLaunchKernelGGL((replan_edge_kernel<D, 4, true, TIMED>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// replan_reserve_kernel<D, K>: the ONE edge (state[pred], U[pred_action]) of every non-root node against the reservation
// table as it is now (include/mplx_replan_timed.h), exactly as reserve_kernel.hip looks at a finite list entry of a row
// whose parent is pred.  One wave per node, four nodes per workgroup; a wave whose node is not looked at leaves at a
// wave-uniform branch.  The lanes are 64 consecutive reservations: pos[d][i][b0 + lane] is one contiguous 512-byte
// request, active[i][b0 + lane] 64 bytes; no LDS, no barrier.  Every lane evaluates the one position of the instant
// (traj::chain_segment / eval_segment in registers, as the check).  Instants ascend in the outer loop and tiles of 64 in
// the inner one, so the first non-zero ballot gives the minimum of (i << 32 | b) directly and ends the wave.  What a lane
// needs of its reservation (its radius, or NaN where it is excluded or of the query's ignored group) is loaded once
// when B <= 64.  The instants are the check's guess and scan of n_scan = ceil(dt / step) + 3.  Loops are bounded by
// n_scan, n_steps and B; no workgroup waits for another; bad[id], hit[id] and the count are written by lane 0 of the
// wave that owns the node (the count by an order-free integer atomic).
constexpr int kWave = 64;
constexpr int kResNodes = kBlock / kWave;
constexpr long long kNoHit = 0x7fffffffffffffffLL;

template <int D, int K>
__global__ __launch_bounds__(kBlock) void replan_reserve_kernel(const ReplanTimedArgs X) {
  const ReplanArgs &R = X.R;
  const ReserveArgs &A = X.res;
  if (R.ctl->status) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t id = (int64_t)blockIdx.x * kResNodes + (threadIdx.x >> 6), n = node_count(R);
  if (id >= n) return;  // (wave-uniform, as every branch on the node below)
  const int32_t p = R.pred[id], a = R.pred_action[id];
  bool look = p >= 0 && p < n && a >= 0 && a < A.nU && !is_root(R, id);
  int32_t q = 0;
  if (look && A.node_query) q = A.node_query[id];
  if (q < 0 || q >= A.Q) {
    look = false;
    q = 0;
  }
  if (!look) {
    if (X.hit && lane == 0) X.hit[id] = -1LL;
    return;
  }
  const double t0 = A.q_t0[q], rq = A.q_r[q];
  const int32_t ign = A.q_ignore[q];
  constexpr int F = 4 * D + 2;
  double ps[4 * D];
#pragma unroll
  for (int f = 0; f < 4 * D; f++) ps[f] = R.state[(int64_t)f * R.cap + p];
  const double tp = R.state[(int64_t)(F - 1) * R.cap + p];
  const double tc = tp + A.dt;
  const bool horizon = (double)(A.n_steps - 1) * A.step - t0 < tc;
  long long key = kNoHit;
  if (!horizon) {
    // the instants [i0, i0 + ni): reserve_check_kernel's guess and scan
    int i0 = 0, ni = 0;
    const double x = (tp + t0) / A.step;
    int64_t g = 0;  // (a NaN goes to 0)
    if (x >= 1.0) g = x < 2147483647.0 ? (int64_t)x - 1 : (int64_t)A.n_steps;
    for (int s = 0; s < A.n_scan; s++) {
      const int64_t i = g + s;
      if (i >= A.n_steps) break;
      const double tl = (double)i * A.step - t0;
      if (tl > tc) break;
      if (tl >= tp) {
        if (ni == 0) i0 = (int)i;
        ni++;
      }
    }
    double seg[5 * D + 2];
    {
      dev::Ax<K> ax[D];
      traj::chain_segment<D, K>(ps, A.U + (int64_t)a * A.udim, 0.0, 0.0, ax, seg, 1);
    }
    const bool one_tile = A.B <= kWave;
    double r0 = NAN;
    if (one_tile && lane < A.B && A.incl[lane] != 0 && A.group[lane] != ign) r0 = A.r[lane];
    for (int ii = 0; ii < ni && key == kNoHit; ii++) {
      const int i = i0 + ii;
      const double tl = (double)i * A.step - t0;
      traj::Sample<D> sm;
      traj::eval_segment<D, true, false>(seg, 1, tl - tp, sm);
      for (int64_t b0 = 0; b0 < A.B; b0 += kWave) {
        const int64_t b = b0 + lane;
        bool conf = false;
        if (b < A.B) {
          const int64_t at = (int64_t)i * A.B + b;
          double rb = one_tile ? r0 : ((A.incl[b] != 0 && A.group[b] != ign) ? A.r[b] : NAN);
          if (A.act[at] == 0) rb = NAN;
          const double dx = sm.pos[0] - A.pos[at], dy = sm.pos[1] - A.pos[(int64_t)A.n_steps * A.B + at];
          double d2 = (dx * dx) + dy * dy;
          if (D == 3) {
            const double dz = sm.pos[D - 1] - A.pos[(int64_t)(D - 1) * A.n_steps * A.B + at];
            d2 = d2 + dz * dz;
          }
          const double rr = rq + rb;
          conf = d2 < rr * rr;  // (a NaN on either side compares false)
        }
        const unsigned long long bal = __ballot(conf);
        if (bal) {
          key = ((long long)i << 32) | (long long)(b0 + (__ffsll((long long)bal) - 1));
          break;
        }
      }
    }
  }
  if (lane != 0) return;
  const bool blocked = horizon || key != kNoHit;
  if (X.hit) X.hit[id] = blocked ? (horizon ? -2LL : key) : -1LL;
  if (blocked) {
    R.bad[id] = 1;  // (OR: the edge pass, an earlier launch, may have set it already)
    if (X.n_blocked) atomicAdd(X.n_blocked, 1ull);
  }
}

template <int D>
hipError_t reserve_dim(int order, const ReplanTimedArgs &a, dim3 grid, hipStream_t s) {
  const dim3 block(kBlock);
  switch (order) {
    case 1: hipLaunchKernelGGL((replan_reserve_kernel<D, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((replan_reserve_kernel<D, 2>), grid, block, 0, s, a); break;
    case 3: hipLaunchKernelGGL((replan_reserve_kernel<D, 3>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((replan_reserve_kernel<D, 4>), grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

// the passes after the bad-edge bytes are final: init, resolve, apply, scan, emit
hipError_t rebase_tail(const ReplanArgs &a, int passes, dim3 per_node, dim3 per_tile, hipStream_t s) {
  const dim3 block(kBlock);
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

}  // namespace

hipError_t launch_replan_rebase(int dim, int control, const ReplanArgs &a, int passes, hipStream_t s) {
  const int64_t n = a.n_bound > 0 ? a.n_bound : 1;
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), per_tile((unsigned)a.n_tiles);
  if (hipError_t e = hipMemsetAsync(a.counters, 0, sizeof(ReplanResult), s)) return e;
  if (a.check_edges) {
    hipError_t e = dim == 2 ? edge_dim<2, false>(control, a, per_node, s) : dim == 3 ? edge_dim<3, false>(control, a, per_node, s) : hipErrorInvalidValue;
    if (e != hipSuccess) return e;
  }
  return rebase_tail(a, passes, per_node, per_tile, s);
}

// The edge pass writes bad[id] for every id (or, without check_edges, a memset clears it); the reservation pass, the
// next launch, ORs into it; the init pass then reads the union.
hipError_t launch_replan_rebase_timed(int dim, int control, const ReplanTimedArgs &a, int passes, hipStream_t s) {
  const ReplanArgs &r = a.R;
  const int64_t n = r.n_bound > 0 ? r.n_bound : 1;
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), per_tile((unsigned)r.n_tiles);
  if (dim != 2 && dim != 3) return hipErrorInvalidValue;
  if (hipError_t e = hipMemsetAsync(r.counters, 0, sizeof(ReplanResult), s)) return e;
  if (r.check_edges) {
    if (hipError_t e = dim == 2 ? edge_dim<2, true>(control, a, per_node, s) : edge_dim<3, true>(control, a, per_node, s)) return e;
  } else if (a.use_res) {
    if (hipError_t e = hipMemsetAsync(r.bad, 0, (size_t)n, s)) return e;
  }
  if (a.use_res) {
    const int ctl = control & 0x0f;
    const int order = ctl == 0x01 ? 1 : ctl == 0x03 ? 2 : ctl == 0x07 ? 3 : ctl == 0x0f ? 4 : 0;
    const dim3 grid((unsigned)((n + kResNodes - 1) / kResNodes));
    if (hipError_t e = dim == 2 ? reserve_dim<2>(order, a, grid, s) : reserve_dim<3>(order, a, grid, s)) return e;
  }
  ReplanArgs t = r;
  t.check_edges = (r.check_edges || a.use_res) ? 1 : 0;  // the init pass reads bad[]
  return rebase_tail(t, passes, per_node, per_tile, s);
}

}  // namespace mplx
