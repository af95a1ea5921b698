// open_kernel.hip -- the open set of a node table (include/mplx_open.h): what GraphSearch::Astar keeps in its priority
// queue (reference include/mpl_planner/common/graph_search.h:53-143: the key g + eps * h, pop the smallest, re-open a
// closed node whose g fell, stop when the goal is at the top), for whole batches on the arrays of table_kernel.hip.
//
// The table's discipline holds here too: a launch boundary is the only ordering between
// passes, no workgroup waits for another, only order-free atomics (min, add) decide anything, and ranks come from prefix
// sums in id order -- every output is a pure function of the inputs.
//
// A push is one lane per frontier row: the fused heuristic and tolerance test of the expansion kernels (dev::post_eval)
// on the row's state, f = g + eps * h, one 8-byte and one 1-byte store per node.  With the ray trace it is two passes
// around the goal passes of ray_kernel.hip, which see the frontier as lists of stride 1.
//
// A select is four launches:
//   reduce   per node: wave minima of f's bit patterns over the open nodes and over the goal-region nodes (non-negative
//            doubles order like uint64, as the table's lower pass uses), one 64-bit atomicMin per wave; both sets counted
//   mark     per tile of 4096 ids: the status from the control block; SELECTED: open nodes with f <= f_min + delta are
//            marked and counted per tile; goal-region nodes with f == goal_f: atomicMin(goal_id)
//   scan     exclusive prefix sums of the tile counts (one workgroup), clamped to the frontier's capacity; the result
//            block, the frontier count, the pinned mirror; resets the control block of the NEXT select
//   emit     marked nodes in id order -> id, g and the state rows gathered from the table; IS_OPEN is cleared for the
//            ranks below the capacity only
// Every index is checked where it is formed: ids against the table's own node count, rows against the frontier's
// capacity.  A table with a status bit makes every pass return at its first instruction.
//
// A table with several queries (include/mplx_multi.h) has one control block, one goal and one result per query.  Its
// push is the same kernel with the goal looked up by the node's query; its select is the *_multi kernels at the end of
// this file: the same four passes with every decision taken per query, and a fifth launch of one lane per query that
// writes the results once the emit pass has counted each query's rows below the frontier's capacity.  The kernels of a
// table with one query are untouched by that.
//
// With priors (include/mplx_prior.h) the push is the same kernel again with the heuristic of a guided query read from the
// open set's prior table (built by traj_kernel.hip); the instantiations without priors are untouched by that.
//
// With a goal field (include/mplx_field.h) it is the same kernel once more: the heuristic of a query with a field takes the
// larger of the default's Linf distance and the grid distance the field holds for the row's cell; the instantiations
// without a field are untouched by that.
//
// With the dynamics-aware heuristic (include/mplx_heur.h) it is the same kernel a last time: heur::robust of
// csrc/mplx_heur_math.h on the row's state and its query's goal, never below the default; with a field the larger of the
// two.  ROBUST only: the reference's closed forms go through cbrt / acos / cos, whose bits are not the host's.  The
// instantiations without it are untouched by that.
#include "mplx_internal.h"
#include "mplx_device_common.h"
#include "mplx_heur_math.h"

namespace mplx {
namespace {

constexpr int kBlock = 256;
constexpr int kItems = kTableTile / kBlock;
constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;
constexpr uint8_t kIsOpen = 1, kIsGoal = 2, kSeen = 4;  // MPLX_OPEN_* of include/mplx_open.h
constexpr int32_t kSelected = 0, kFound = 1, kEmpty = 2;
constexpr uint8_t kRowTol = 1, kRowBlocked = 8, kRowCounts = 0x80;

__device__ __forceinline__ int64_t node_count(const OpenArgs &A) {
  const int64_t n = A.t_ctl->n_nodes;
  return n < 0 ? 0 : (n < A.cap ? n : A.cap);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(v >> 32), d) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)v, d);
    v = o < v ? o : v;
  }
  return v;
}

// What the control block decides once the reduce pass is complete.
struct Decision {
  int32_t status;
  double f_min, goal_f, T;
  unsigned long long goalf_bits;
  bool any_goal;
};
__device__ __forceinline__ Decision decide(const OpenCtl *c, double delta) {
  Decision d;
  const uint32_t n_open = c->n_open;
  d.any_goal = c->n_goal != 0;
  d.goalf_bits = c->goalf_bits;
  d.f_min = __longlong_as_double((long long)c->fmin_bits);
  d.goal_f = __longlong_as_double((long long)d.goalf_bits);
  d.status = (d.any_goal && d.goal_f <= d.f_min) ? kFound : n_open == 0 ? kEmpty : kSelected;
  d.T = d.f_min + delta;
  return d;
}
__device__ __forceinline__ Decision decide(const OpenArgs &A) { return decide(A.ctl, A.delta); }

// MULTI: the goal is goals[query of the node] (mplx_open_set_goals), not the context's
// CLOSED: the push of include/mplx_replan.h -- key and goal bit as ever, but the node is not opened
// PRIOR: include/mplx_prior.h -- a query with a prior table takes its heuristic from where the prior is at the row's time
// (env_base.h:46-53); the instantiations without it are the kernels they were
// FIELD: include/mplx_field.h -- a query with a goal field takes max(Linf, res * (dist - 1)) where the default takes Linf,
// and +inf on a cell no chain leaves; likewise
// DYN: include/mplx_heur.h -- h = max(heur::robust, what the kernel had); a NaN (non-finite rows) makes the row ignored; likewise
template <int D, bool MULTI, bool CLOSED, bool PRIOR, bool FIELD, bool DYN>
__global__ __launch_bounds__(kBlock) void open_push_kernel(const OpenArgs A, int64_t rows, int pass) {
  if (A.t_ctl->status) return;
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= rows) return;  // rows <= min(n_max, f_cap): the host's bound
  if (pass == 0 && A.row_flags) {
    A.row_flags[r] = 0;
    A.row_count[r] = 1;
  }
  int64_t n = *A.f_count;
  n = n < A.n_max ? n : A.n_max;
  n = n < A.f_cap ? n : A.f_cap;
  if (r >= n) return;
  const int64_t id = A.f_id[r];
  if (id < 0 || id >= node_count(A)) return;
  if (pass == 1) {
    const uint8_t rf = A.row_flags[r];
    if (rf & kRowCounts) A.flags[id] = (uint8_t)(kSeen | (CLOSED ? 0 : kIsOpen) | (((rf & kRowTol) && !(rf & kRowBlocked)) ? kIsGoal : 0));
    return;
  }
  double s[4 * D + 1];
#pragma unroll
  for (int i = 0; i < 3 * D; i++) s[i] = A.f_state[(int64_t)i * A.f_stride + r];
  s[4 * D] = A.f_state[(int64_t)(4 * D) * A.f_stride + r];
  const double t_row = PRIOR ? A.f_state[(int64_t)(4 * D + 1) * A.f_stride + r] : 0.0;
  int32_t q = 0;
  if (MULTI && A.t_query) {
    q = A.t_query[id];
    if (q < 0 || q >= A.n_queries) return;  // (never: the column holds only queries)
  }
  const PostFuse &GF = MULTI ? A.goals[q] : A.goal;
  MPLX_POST_GOAL(PG, GF, D)
  double h;
  unsigned int fl;
  dev::post_eval<D>(PG, A.t_hash[id], s, s + D, s + 2 * D, s[4 * D], &h, &fl);
  double h_dyn = 0.0;
  if (DYN && !(fl & 2u)) {  // (bit 1: the goal's own lattice state keeps h = 0, env_base.h:47)
    const int32_t *ctl = (MULTI && A.dyn_controls) ? A.dyn_controls + 2 * (int64_t)q : A.dyn_control;
    h_dyn = heur::robust<D>(s, PG.g, ctl[0], ctl[1], PG.w, PG.v_max);
  }
  if (PRIOR && !(fl & 2u)) {  // (bit 1: the goal's own lattice state keeps h = 0, env_base.h:47)
    const int32_t ns = A.prior_n[q];
    const double x = t_row > 0 ? t_row / A.prior_dt : 0.0;  // env_base.h:48
    if (ns > 0 && x < (double)ns) {
      int64_t k = (int64_t)x;
      k = k < 0 ? 0 : (k < A.prior_cap ? k : A.prior_cap - 1);  // (0 <= x < ns <= prior_cap: never moves)
      const double *pp = A.prior_pos + ((int64_t)q * A.prior_cap + k) * D;
      double m = 0;
#pragma unroll
      for (int i = 0; i < D; i++) {
        const double d = fabs(s[i] - pp[i]);
        m = d > m ? d : m;
      }
      const double lin = PG.v_max > 0 ? PG.w * m / PG.v_max : PG.w * m;
      h = lin + A.prior_togo[(int64_t)q * A.prior_cap + k];
    }
  }
  if (FIELD && !(fl & 2u)) {  // (bit 1: the goal's own lattice state keeps h = 0)
    const int32_t fq = A.field_of_query[q];
    if (fq >= 0 && fq < A.field_F) {  // (the host checked the entries: never out of range)
      bool inside = true;
      int64_t idx = 0, mul = 1;
#pragma unroll
      for (int i = 0; i < D; i++) {
        const double c = round((s[i] - A.field_org[i]) / A.field_res - 0.5);  // map_util.h:103-108
        const bool in = c >= 0.0 && c < (double)A.field_dim[i];  // compared as a double: NaN and huge values are outside
        inside = inside && in;
        idx += (in ? (int64_t)c : 0) * mul;
        mul *= A.field_dim[i];
      }
      const int32_t n = inside ? A.field_dist[(int64_t)fq * A.field_cells + idx] : -1;
      if (n < 0) {
        h = __longlong_as_double((long long)kInfBits);
      } else {
        double L = 0;  // post_eval's lpNorm<Infinity> of pos - goal.pos
#pragma unroll
        for (int i = 0; i < D; i++) {
          const double d = fabs(s[i] - PG.g[i]);
          L = d > L ? d : L;
        }
        const double G = A.field_res * (double)(n - 1 > 0 ? n - 1 : 0);
        if (G > L) h = PG.v_max > 0 ? PG.w * G / PG.v_max : PG.w * G;  // (G <= L: post_eval's h, bit for bit)
      }
    }
  }
  if (DYN && !(h_dyn <= h)) h = h_dyn;  // the larger; a NaN stays
  const double g = A.f_g[r];
  double f = g;
  if (A.eps != 0.0) {
    const double eh = A.eps * h;
    f = g + eh;
  }
  if (!(f >= 0.0)) return;
  f = f + 0.0;  // -0.0 -> +0.0: the bit patterns of the keys order like the keys
  A.f[id] = (unsigned long long)__double_as_longlong(f);
  if (A.row_flags) {
    A.row_flags[r] = (uint8_t)(kRowCounts | (fl & 1u));
    if (MULTI) A.row_query[r] = q;
  } else A.flags[id] = (uint8_t)(kSeen | (CLOSED ? 0 : kIsOpen) | ((fl & 1u) ? kIsGoal : 0));
}

__global__ __launch_bounds__(kBlock) void open_reduce_kernel(const OpenArgs A) {
  if (A.t_ctl->status) return;  // (uniform)
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long fo = kInfBits, fg = kInfBits;
  bool o = false, g = false;
  if (id < node_count(A)) {
    const uint8_t fl = A.flags[id];
    o = (fl & kIsOpen) != 0;
    g = (fl & kIsGoal) != 0;
    if (o || g) {
      const unsigned long long v = A.f[id];
      if (o) fo = v;
      if (g) fg = v;
    }
  }
  const unsigned long long bo = __ballot(o), bg = __ballot(g);  // the wave's sets, in every lane
  if (bo) fo = wave_min(fo);
  if (bg) fg = wave_min(fg);
  if ((threadIdx.x & 63) != 0) return;
  if (bo) {
    atomicMin(&A.ctl->fmin_bits, fo);
    atomicAdd(&A.ctl->n_open, (uint32_t)__popcll(bo));
  }
  if (bg) {
    atomicMin(&A.ctl->goalf_bits, fg);
    atomicAdd(&A.ctl->n_goal, (uint32_t)__popcll(bg));
  }
}

__global__ __launch_bounds__(kBlock) void open_mark_kernel(const OpenArgs A) {
  if (A.t_ctl->status) return;  // (uniform: nothing below is skipped by part of a workgroup)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = node_count(A), base = (int64_t)blockIdx.x * kTableTile;
  const Decision d = decide(A);
  uint32_t cnt = 0;
  for (int i = 0; i < kItems; i++) {
    const int64_t id = base + (int64_t)i * kBlock + threadIdx.x;
    bool m = false;
    if (id < n) {
      const uint8_t fl = A.flags[id];
      if (fl & (kIsOpen | kIsGoal)) {
        const unsigned long long v = A.f[id];
        if ((fl & kIsGoal) && v == d.goalf_bits) atomicMin(&A.ctl->goal_id, (int32_t)id);
        m = d.status == kSelected && (fl & kIsOpen) && __longlong_as_double((long long)v) <= d.T;
      }
      A.mark[id] = m ? 1 : 0;
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

// table_scan_kernel's scan of the tile counts, then the result of the select.
__global__ __launch_bounds__(1024) void open_scan_kernel(const OpenArgs A) {
  __shared__ uint32_t part[1024];
  if (A.t_ctl->status) return;  // (uniform)
  const int t = threadIdx.x;
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
  if (t != 0) return;
  const Decision d = decide(A);
  int64_t cnt = 0;
  if (d.status == kSelected) {
    cnt = part[1023];
    if (cnt > A.f_cap) cnt = A.f_cap;  // the rest stay open
  }
  A.ctl->emit = cnt > 0 ? 1 : 0;
  *A.f_count = cnt;
  OpenResult R;
  R.status = d.status;
  R.goal_id = d.any_goal ? A.ctl->goal_id : -1;
  R.count = cnt;
  R.n_open = (int64_t)A.ctl->n_open - cnt;
  R.f_min = d.f_min;
  R.goal_f = d.goal_f;
  R.goal_g = (R.goal_id >= 0 && R.goal_id < node_count(A)) ? __longlong_as_double((long long)A.t_g[R.goal_id]) : __longlong_as_double((long long)kInfBits);
  if (A.result) *A.result = R;
  // the pinned mirror: what the host reads, without a copy, once it has waited for the stream
  __hip_atomic_store(&A.mirror->goal_id, R.goal_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&A.mirror->count, R.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&A.mirror->n_open, R.n_open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&A.mirror->f_min, R.f_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&A.mirror->goal_f, R.goal_f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&A.mirror->goal_g, R.goal_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&A.mirror->status, R.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  // the next select reduces into the other control block (this one is read by the emit pass behind this launch)
  A.ctl_next->fmin_bits = kInfBits;
  A.ctl_next->goalf_bits = kInfBits;
  A.ctl_next->n_open = 0;
  A.ctl_next->n_goal = 0;
  A.ctl_next->goal_id = 0x7fffffff;
  A.ctl_next->emit = 0;
  A.ctl_next->n_sel = 0;
}

// Rank of every marked node of a tile in id order = its frontier row.
__global__ __launch_bounds__(kBlock) void open_emit_kernel(const OpenArgs A) {
  if (A.t_ctl->status || A.ctl->emit == 0) return;  // (uniform)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = node_count(A), base = (int64_t)blockIdx.x * kTableTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t run = A.tot[blockIdx.x];
  for (int i = 0; i < kItems; i++) {
    const int64_t id = base + (int64_t)i * kBlock + threadIdx.x;
    const bool m = id < n && A.mark[id] != 0;
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
    if (!m || r >= A.f_cap) continue;
    A.flags[id] = (uint8_t)(A.flags[id] & ~kIsOpen);
    A.f_id[r] = (int32_t)id;
    A.f_g[r] = __longlong_as_double((long long)A.t_g[id]);
    for (int f = 0; f < A.n_fields; f++) A.f_state[(int64_t)f * A.f_stride + r] = A.t_state[(int64_t)f * A.cap + id];
  }
}

__device__ __forceinline__ void reset_ctl(OpenCtl *c) {
  c->fmin_bits = kInfBits;
  c->goalf_bits = kInfBits;
  c->n_open = 0;
  c->n_goal = 0;
  c->goal_id = 0x7fffffff;
  c->emit = 0;
  c->n_sel = 0;
  c->pad = 0;
}

// both halves: n_queries control blocks each
__global__ __launch_bounds__(kBlock) void open_clear_kernel(const OpenArgs A) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= A.n_queries) return;
  reset_ctl(A.ctl + q);
  reset_ctl(A.ctl_next + q);
}

// ---- select on a table with several queries ------------------------------------------------------------------------

__device__ __forceinline__ int32_t query_of(const OpenArgs &A, int64_t id) {
  if (!A.t_query) return 0;
  const int32_t q = A.t_query[id];
  return (q >= 0 && q < A.n_queries) ? q : 0;  // (the column holds only queries: no index leaves the control blocks)
}

__device__ __forceinline__ Decision decide_query(const OpenArgs &A, int32_t q) { return decide(A.ctl + q, A.delta); }

// `on` lanes share query q (wave-uniform): the wave's minimum and count go to that query with one atomic each.  Every
// lane of the wave calls this.
__device__ __forceinline__ void reduce_one(const OpenArgs &A, int32_t q, bool o, bool g, unsigned long long f) {
  const unsigned long long bo = __ballot(o), bg = __ballot(g);
  unsigned long long fo = o ? f : kInfBits, fg = g ? f : kInfBits;
  if (bo) fo = wave_min(fo);
  if (bg) fg = wave_min(fg);
  if ((threadIdx.x & 63) != 0) return;
  OpenCtl *c = A.ctl + q;
  if (bo) {
    atomicMin(&c->fmin_bits, fo);
    atomicAdd(&c->n_open, (uint32_t)__popcll(bo));
  }
  if (bg) {
    atomicMin(&c->goalf_bits, fg);
    atomicAdd(&c->n_goal, (uint32_t)__popcll(bg));
  }
}

__global__ __launch_bounds__(kBlock) void open_reduce_multi_kernel(const OpenArgs A) {
  if (A.t_ctl->status) return;  // (uniform)
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  unsigned long long f = kInfBits;
  bool o = false, g = false;
  int32_t q = 0;
  if (id < node_count(A)) {
    const uint8_t fl = A.flags[id];
    o = (fl & kIsOpen) != 0;
    g = (fl & kIsGoal) != 0;
    if (o || g) {
      f = A.f[id];
      q = query_of(A, id);
    }
  }
  unsigned long long left = __ballot(o || g);  // the lanes with something to say
  if (!left) return;
  const int32_t q0 = __shfl(q, __builtin_ctzll(left));
  if (__ballot((o || g) && q != q0) == 0ull) {  // one query in the wave: the pass of a table with one query
    reduce_one(A, q0, o, g, f);
    return;
  }
  while (left) {  // one round per distinct query present, at most 64
    const int32_t qq = __shfl(q, __builtin_ctzll(left));
    const bool mine = (o || g) && q == qq;
    reduce_one(A, qq, mine && o, mine && g, f);
    left &= ~__ballot(mine);
  }
}

__global__ __launch_bounds__(kBlock) void open_mark_multi_kernel(const OpenArgs A) {
  if (A.t_ctl->status) return;  // (uniform: nothing below is skipped by part of a workgroup)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = node_count(A), base = (int64_t)blockIdx.x * kTableTile;
  uint32_t cnt = 0;
  for (int i = 0; i < kItems; i++) {
    const int64_t id = base + (int64_t)i * kBlock + threadIdx.x;
    bool m = false;
    if (id < n) {
      const uint8_t fl = A.flags[id];
      if (fl & (kIsOpen | kIsGoal)) {
        const int32_t q = query_of(A, id);
        const Decision d = decide_query(A, q);  // the node's own query decides
        const unsigned long long v = A.f[id];
        if ((fl & kIsGoal) && v == d.goalf_bits) atomicMin(&A.ctl[q].goal_id, (int32_t)id);
        m = d.status == kSelected && (fl & kIsOpen) && __longlong_as_double((long long)v) <= d.T;
      }
      A.mark[id] = m ? 1 : 0;
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

// The scan of the tile counts; the frontier count (the marks are those of the SELECTED queries only) clamped to the
// capacity; the control blocks of the NEXT select.  The results wait for the emit pass's counts (open_finish_kernel).
__global__ __launch_bounds__(1024) void open_scan_multi_kernel(const OpenArgs A) {
  __shared__ uint32_t part[1024];
  if (A.t_ctl->status) return;  // (uniform)
  const int t = threadIdx.x;
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
  for (int32_t q = t; q < A.n_queries; q += 1024) reset_ctl(A.ctl_next + q);
  if (t != 0) return;
  int64_t cnt = part[1023];
  if (cnt > A.f_cap) cnt = A.f_cap;  // the rest stay open
  A.ctl[0].emit = cnt > 0 ? 1 : 0;  // (query 0's block carries the flag of the whole select)
  *A.f_count = cnt;
}

// open_emit_kernel, and per (wave, query) one atomicAdd of the rows emitted: integer sums, the same whatever the order.
__global__ __launch_bounds__(kBlock) void open_emit_multi_kernel(const OpenArgs A) {
  if (A.t_ctl->status || A.ctl[0].emit == 0) return;  // (uniform)
  __shared__ uint32_t wsum[kBlock / 64];
  const int64_t n = node_count(A), base = (int64_t)blockIdx.x * kTableTile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t run = A.tot[blockIdx.x];
  for (int i = 0; i < kItems; i++) {
    const int64_t id = base + (int64_t)i * kBlock + threadIdx.x;
    const bool m = id < n && A.mark[id] != 0;
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
    const bool take = m && r < A.f_cap;
    int32_t q = 0;
    if (take) {
      q = query_of(A, id);
      A.flags[id] = (uint8_t)(A.flags[id] & ~kIsOpen);
      A.f_id[r] = (int32_t)id;
      A.f_g[r] = __longlong_as_double((long long)A.t_g[id]);
      for (int f = 0; f < A.n_fields; f++) A.f_state[(int64_t)f * A.f_stride + r] = A.t_state[(int64_t)f * A.cap + id];
    }
    unsigned long long left = __ballot(take);
    while (left) {  // one round per distinct query among the wave's rows (one, when the wave holds one query)
      const int32_t qq = __shfl(q, __builtin_ctzll(left));
      const unsigned long long mine = __ballot(take && q == qq);
      if (lane == 0) atomicAdd(&A.ctl[qq].n_sel, (uint32_t)__popcll(mine));
      left &= ~mine;
    }
  }
}

// One lane per query: the result, to the caller's device memory and to the pinned mirror.
__global__ __launch_bounds__(kBlock) void open_finish_kernel(const OpenArgs A) {
  if (A.t_ctl->status) return;
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= A.n_queries) return;
  const Decision d = decide_query(A, (int32_t)q);
  const OpenCtl *c = A.ctl + q;
  OpenResult R;
  R.status = d.status;
  R.goal_id = d.any_goal ? c->goal_id : -1;
  R.count = d.status == kSelected ? (int64_t)c->n_sel : 0;
  R.n_open = (int64_t)c->n_open - R.count;
  R.f_min = d.f_min;
  R.goal_f = d.goal_f;
  R.goal_g = (R.goal_id >= 0 && R.goal_id < node_count(A)) ? __longlong_as_double((long long)A.t_g[R.goal_id]) : __longlong_as_double((long long)kInfBits);
  if (A.result) A.result[q] = R;
  OpenResult *m = A.mirror + q;
  __hip_atomic_store(&m->goal_id, R.goal_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->count, R.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->n_open, R.n_open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->f_min, R.f_min, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->goal_f, R.goal_f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->goal_g, R.goal_g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->status, R.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

hipError_t launch_open_clear(const OpenArgs &a, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(a.flags, 0, (size_t)a.cap, s)) return e;
  hipLaunchKernelGGL(open_clear_kernel, dim3((unsigned)((a.n_queries + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <int D, bool MULTI, bool PRIOR = false, bool FIELD = false, bool DYN = false>
void push_closed(bool closed, dim3 grid, dim3 block, hipStream_t s, const OpenArgs &a, int64_t rows, int pass) {
  if (closed) hipLaunchKernelGGL((open_push_kernel<D, MULTI, true, PRIOR, FIELD, DYN>), grid, block, 0, s, a, rows, pass);
  else hipLaunchKernelGGL((open_push_kernel<D, MULTI, false, PRIOR, FIELD, DYN>), grid, block, 0, s, a, rows, pass);
}

// include/mplx_heur.h: never together with priors (open_api.cpp)
template <int D>
void push_dyn(bool closed, dim3 grid, dim3 block, hipStream_t s, const OpenArgs &a, int64_t rows, int pass) {
  if (a.field_dist) {
    if (a.goals) push_closed<D, true, false, true, true>(closed, grid, block, s, a, rows, pass);
    else push_closed<D, false, false, true, true>(closed, grid, block, s, a, rows, pass);
  } else {
    if (a.goals) push_closed<D, true, false, false, true>(closed, grid, block, s, a, rows, pass);
    else push_closed<D, false, false, false, true>(closed, grid, block, s, a, rows, pass);
  }
}

hipError_t launch_open_push(int dim, int pass, const OpenArgs &a, int64_t rows, hipStream_t s, bool closed) {
  if (rows <= 0) return hipSuccess;
  const dim3 grid((unsigned)((rows + kBlock - 1) / kBlock)), block(kBlock);
  if (dim != 2 && dim != 3) return hipErrorInvalidValue;
  if (a.dyn) {
    if (a.dyn != 2 || a.prior_n || (a.goals && !a.dyn_controls)) return hipErrorInvalidValue;  // MPLX_HEUR_ROBUST
    if (a.field_dist && (!a.field_of_query || a.field_F < 1 || a.field_cells < 1 || !(a.field_res > 0))) return hipErrorInvalidValue;
    if (dim == 2) push_dyn<2>(closed, grid, block, s, a, rows, pass);
    else push_dyn<3>(closed, grid, block, s, a, rows, pass);
  } else if (a.field_dist) {  // (never together with priors: open_api.cpp)
    if (a.prior_n || !a.field_of_query || a.field_F < 1 || a.field_cells < 1 || !(a.field_res > 0)) return hipErrorInvalidValue;
    if (a.goals) {
      if (dim == 2) push_closed<2, true, false, true>(closed, grid, block, s, a, rows, pass);
      else push_closed<3, true, false, true>(closed, grid, block, s, a, rows, pass);
    } else {
      if (dim == 2) push_closed<2, false, false, true>(closed, grid, block, s, a, rows, pass);
      else push_closed<3, false, false, true>(closed, grid, block, s, a, rows, pass);
    }
  } else if (a.prior_n) {  // (priors need goals of the open set's own: open_api.cpp)
    if (!a.goals || !a.prior_pos || !a.prior_togo || a.prior_cap < 1) return hipErrorInvalidValue;
    if (dim == 2) push_closed<2, true, true>(closed, grid, block, s, a, rows, pass);
    else push_closed<3, true, true>(closed, grid, block, s, a, rows, pass);
  } else if (a.goals) {
    if (dim == 2) push_closed<2, true>(closed, grid, block, s, a, rows, pass);
    else push_closed<3, true>(closed, grid, block, s, a, rows, pass);
  } else {
    if (dim == 2) push_closed<2, false>(closed, grid, block, s, a, rows, pass);
    else push_closed<3, false>(closed, grid, block, s, a, rows, pass);
  }
  return hipGetLastError();
}

hipError_t launch_open_select(const OpenArgs &a, hipStream_t s) {
  const int64_t n = a.n_bound > 0 ? a.n_bound : 1;  // (an empty table still gets its result)
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), per_tile((unsigned)a.n_tiles), block(kBlock);
  hipLaunchKernelGGL(open_reduce_kernel, per_node, block, 0, s, a);
  hipLaunchKernelGGL(open_mark_kernel, per_tile, block, 0, s, a);
  hipLaunchKernelGGL(open_scan_kernel, dim3(1), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(open_emit_kernel, per_tile, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_open_select_multi(const OpenArgs &a, hipStream_t s) {
  const int64_t n = a.n_bound > 0 ? a.n_bound : 1;  // (an empty table still gets its results)
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), per_tile((unsigned)a.n_tiles), block(kBlock);
  hipLaunchKernelGGL(open_reduce_multi_kernel, per_node, block, 0, s, a);
  hipLaunchKernelGGL(open_mark_multi_kernel, per_tile, block, 0, s, a);
  hipLaunchKernelGGL(open_scan_multi_kernel, dim3(1), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(open_emit_multi_kernel, per_tile, block, 0, s, a);
  hipLaunchKernelGGL(open_finish_kernel, dim3((unsigned)((a.n_queries + kBlock - 1) / kBlock)), block, 0, s, a);
  return hipGetLastError();
}

// include/mplx_best.h: the reduce pass in front of the launches of open_best_kernel.hip and the tail of select_multi
// behind them -- the kernels above as they are, launched from here because they are this file's own.
hipError_t launch_open_reduce_only(const OpenArgs &a, bool multi, hipStream_t s) {
  const int64_t n = a.n_bound > 0 ? a.n_bound : 1;
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  if (multi) hipLaunchKernelGGL(open_reduce_multi_kernel, per_node, block, 0, s, a);
  else hipLaunchKernelGGL(open_reduce_kernel, per_node, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_open_tail_multi(const OpenArgs &a, hipStream_t s) {
  const dim3 per_tile((unsigned)a.n_tiles), block(kBlock);
  hipLaunchKernelGGL(open_scan_multi_kernel, dim3(1), dim3(1024), 0, s, a);
  hipLaunchKernelGGL(open_emit_multi_kernel, per_tile, block, 0, s, a);
  hipLaunchKernelGGL(open_finish_kernel, dim3((unsigned)((a.n_queries + kBlock - 1) / kBlock)), block, 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
