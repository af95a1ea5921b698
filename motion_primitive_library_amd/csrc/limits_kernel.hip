// limits_kernel.hip -- caller-given segments into the table of an mplx_poly, and Primitive::max_vel / max_acc / max_jrk
// and validate_primitive on the set a table holds, for gfx950 (MI355X) (include/mplx_limits.h; reference
// include/mpl_basis/primitive.h:152-193, 309-313, 353-394, 450-496, include/mpl_basis/math.h:21-66, 117-131).
//
// poly_load_kernel<D>: one lane per problem, the shape of solve_kernel.  The durations are checked first, so a failed
// problem writes its status only; then the segment rows, taus by sequential addition, and the waypoints as
// eval_segment gives them (segment s at 0.0, the last segment at its duration).
//
// poly_limits_kernel<D, ALL>: one lane per (problem, segment), problem-minor, so a wave reads every coefficient row
// coalesced.  The 3 D maxima of the segment go to the poly's scratch rows (the workspace of the elimination, dead after a
// solve).  poly_limits_reduce_kernel<D>: one lane per problem walks its segments in order: the running maxima, the
// validity of each segment from its maxima and the limits, the first bad segment.  Two launches instead of atomics: every
// output is written once, by one lane, from values that do not depend on the schedule.
//
// Register audit (-Rpass-analysis=kernel-resource-usage) in DESIGN.md 4.16; no LDS, no scratch.
//
// Bit-exactness: -ffp-contract=off; the arithmetic is mplx_limits_math.h.  cbrt, acos and cos are the device library's.
#include "mplx_internal.h"
#include "mplx_limits_math.h"
#include "mplx_traj_device.h"

namespace mplx {
namespace {

constexpr int kBlock = 256;
constexpr int kLoadBlock = 64;  // one wave: K problems spread over as many CUs as K / 64 allows (as solve_kernel)

template <int D>
__global__ __launch_bounds__(kLoadBlock) void poly_load_kernel(const PolyLoadArgs P) {
  constexpr int F = 4 * D + 2, NC = 6 * D + 2;
  const int64_t k = (int64_t)blockIdx.x * kLoadBlock + threadIdx.x;
  if (k >= P.n_prob) return;
  const int64_t n = P.n_prob, wmax = P.w_max;
  int S;
  uint8_t status = 0;
  if (P.src_index) {  // the gather form: the indices up to the first -1, every one a src problem that holds a segment
    S = 0;
    while (S < P.w_max - 1) {
      const int32_t q = P.src_index[(int64_t)S * P.index_stride + k];
      if (q == -1) break;
      if (q < 0 || q >= P.src_n || P.src_S[q] < 1) {
        status = 1;
        break;
      }
      S++;
    }
    if (S < 1) status = 1;  // MPLX_SOLVE_EMPTY
  } else {
    S = P.n_segs ? P.n_segs[k] : P.w_max - 1;
    if (S > P.w_max - 1) S = P.w_max - 1;
    status = S < 1 ? 1 : 0;  // MPLX_SOLVE_EMPTY
    for (int s = 0; s < S; s++) {
      const double T = P.dts[(int64_t)s * P.dt_stride + k];
      if (!(T > 0.0) || !isfinite(T)) status = 2;  // MPLX_SOLVE_BAD_TIME
    }
  }
  P.tab_status[k] = status;
  if (P.status) P.status[k] = status;
  if (status) {  // a failed problem: its status only; samples, traversals and limits skip it (S = 0)
    P.tab_S[k] = 0;
    P.tab_T[k] = 0.0;
    return;
  }
  double tau = 0.0;
  for (int s = 0; s < S; s++) {
    double T;
    double *seg = P.tab_seg + (int64_t)s * NC * n + k;
    if (P.src_index) {  // segment 0 of problem q of the source table, row for row
      const int64_t q = P.src_index[(int64_t)s * P.index_stride + k];
      T = P.src_dt[q];
#pragma unroll
      for (int r = 0; r < NC; r++) seg[(int64_t)r * n] = P.src_seg[(int64_t)r * P.src_n + q];
    } else {
      T = P.dts[(int64_t)s * P.dt_stride + k];
      const double *src = P.coeff + (int64_t)s * (D + 1) * 6 * P.coeff_stride + k;
#pragma unroll
      for (int r = 0; r < 6 * D; r++) seg[(int64_t)r * n] = src[(int64_t)r * P.coeff_stride];
      seg[(int64_t)(6 * D) * n] = src[(int64_t)(6 * D + 4) * P.coeff_stride];
      seg[(int64_t)(6 * D + 1) * n] = src[(int64_t)(6 * D + 5) * P.coeff_stride];
    }
    P.tab_dt[(int64_t)s * n + k] = T;
    P.tab_tau[(int64_t)s * n + k] = tau;
    if (P.taus_out) P.taus_out[(int64_t)s * P.taus_stride + k] = tau;
    // the waypoint the segment starts from and, for the last one, the waypoint it ends in (the stores above are this
    // lane's own: it reads them back)
    for (int e = 0; e < (s == S - 1 ? 2 : 1); e++) {
      traj::Sample<D> sm;
      traj::eval_segment<D, false, true, true>(seg, n, e ? T : 0.0, sm);
      const double t = e ? tau + T : tau;
      double *wp = P.tab_wp + (int64_t)(s + e) * n + k;
#pragma unroll
      for (int i = 0; i < D; i++) {
        wp[(int64_t)(0 * D + i) * wmax * n] = sm.pos[i];
        wp[(int64_t)(1 * D + i) * wmax * n] = sm.vel[i];
        wp[(int64_t)(2 * D + i) * wmax * n] = sm.acc[i];
        wp[(int64_t)(3 * D + i) * wmax * n] = sm.jrk[i];
      }
      wp[(int64_t)(4 * D) * wmax * n] = sm.yaw;
      wp[(int64_t)(F - 1) * wmax * n] = t;
    }
    tau = tau + T;  // poly_traj.cpp:67
  }
  P.tab_tau[(int64_t)S * n + k] = tau;
  P.tab_S[k] = S;
  P.tab_T[k] = tau;
  if (P.taus_out) P.taus_out[(int64_t)S * P.taus_stride + k] = tau;
  if (P.n_segs_out) P.n_segs_out[k] = S;
  if (P.total_time) P.total_time[k] = tau;
}

template <int D, bool ALL>
__global__ __launch_bounds__(kBlock) void poly_limits_kernel(const LimitsArgs P) {
  constexpr int NC = 6 * D + 2;
  const int64_t n = P.n_prob;
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= n * P.s_max) return;
  const int64_t s = g / n, k = g - s * n;
  if (s >= P.tab_S[k]) return;
  const double *seg = P.tab_seg + s * NC * n + k;
  const double T = P.tab_dt[s * n + k];
  double *o = P.seg_max + s * (3 * D) * n + k;
#pragma unroll
  for (int i = 0; i < D; i++) {
    double c[6];
#pragma unroll
    for (int j = 0; j < 6; j++) c[j] = seg[(int64_t)(6 * i + j) * n];
    o[(int64_t)(0 * D + i) * n] = limits::axis_max<1, ALL>(c, T);
    o[(int64_t)(1 * D + i) * n] = limits::axis_max<2, ALL>(c, T);
    o[(int64_t)(2 * D + i) * n] = limits::axis_max<3, ALL>(c, T);
  }
}

template <int D>
__global__ __launch_bounds__(kBlock) void poly_limits_reduce_kernel(const LimitsArgs P) {
  const int64_t n = P.n_prob;
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  const int S = P.tab_S[k];
  if (S == 0) return;  // a failed problem: the caller's bytes stay
  // validate_primitive, primitive.h:450-475: what the control checks; validate_xxx passes for a limit <= 0
  const int order = P.control & 0x0f;
  const double lim[3] = {P.mv, P.ma, P.mj};
  const bool chk[3] = {order >= 0x03 && !(P.mv <= 0), order >= 0x07 && !(P.ma <= 0), order >= 0x0f && !(P.mj <= 0)};
  double m[3][D];
  int first_bad = -1;
  for (int s = 0; s < S; s++) {
    const double *sm = P.seg_max + (int64_t)s * (3 * D) * n + k;
    bool ok = true;
#pragma unroll
    for (int q = 0; q < 3; q++)
#pragma unroll
      for (int i = 0; i < D; i++) {
        const double x = sm[(int64_t)(q * D + i) * n];
        m[q][i] = (s == 0 || x > m[q][i]) ? x : m[q][i];
        if (chk[q] && x > lim[q]) ok = false;
      }
    if (!ok && first_bad < 0) first_bad = s;
  }
  uint8_t exceed = 0;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    double top = m[q][0];
#pragma unroll
    for (int i = 1; i < D; i++) top = m[q][i] > top ? m[q][i] : top;
    if (!(lim[q] <= 0) && top > lim[q]) exceed |= (uint8_t)(1u << q);
    double *dst = q == 0 ? P.max_vel : (q == 1 ? P.max_acc : P.max_jrk);
    if (dst) {
#pragma unroll
      for (int i = 0; i < D; i++) dst[(int64_t)i * P.max_stride + k] = m[q][i];
    }
  }
  if (P.exceed) P.exceed[k] = exceed;
  if (P.valid) P.valid[k] = first_bad < 0 ? 1 : 0;
  if (P.first_bad) P.first_bad[k] = first_bad;
}

// ---- shortcutting (include/mplx_limits.h) ----
// shortcut_pairs_kernel<D>: one lane per pair p = (k (w_max - 1) + i) max_hop + (j - i - 1): the two-waypoint problem
// from state i to state j of query k for mplx_solve_device: both rows copied as they are, every use bit set (the solver
// masks them to its order), duration t_j - t_i, n_wp = 2, or 0 where j is past the chain.
template <int D>
__global__ __launch_bounds__(kBlock) void shortcut_pairs_kernel(const ShortcutArgs P) {
  constexpr int F = 4 * D + 2;
  const int64_t NP = P.n_query * (P.w_max - 1) * P.max_hop;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= NP) return;
  const int64_t ki = p / P.max_hop;
  const int h = (int)(p - ki * P.max_hop);
  const int64_t k = ki / (P.w_max - 1);
  const int i = (int)(ki - k * (P.w_max - 1)), j = i + h + 1;
  int W = P.n_wp ? P.n_wp[k] : P.w_max;
  if (W > P.w_max) W = P.w_max;
  P.pair_flags[p] = 7;
  P.pair_flags[NP + p] = 7;
  if (j >= W) {
    P.pair_nwp[p] = 0;
    P.pair_dt[p] = 0.0;
    return;
  }
  const double *a = P.states + (int64_t)i * P.stride + k, *b = P.states + (int64_t)j * P.stride + k;
  const int64_t fs = (int64_t)P.w_max * P.stride;
#pragma unroll
  for (int f = 0; f < F; f++) {
    P.pair_wp[((int64_t)f * 2 + 0) * NP + p] = a[f * fs];
    P.pair_wp[((int64_t)f * 2 + 1) * NP + p] = b[f * fs];
  }
  P.pair_nwp[p] = 2;
  P.pair_dt[p] = b[(F - 1) * fs] - a[(F - 1) * fs];
}

// shortcut_cost_kernel: one lane per pair: c[i][j] = (J + w T) + trav, +inf where the edge is not admitted; an adjacent
// edge is always admitted (a trav that is not finite counts as 0.0) unless its solve failed: then NaN, which the
// programme reads as a bad chain.
__global__ __launch_bounds__(kBlock) void shortcut_cost_kernel(const ShortcutArgs P) {
  const int64_t NP = P.n_query * (P.w_max - 1) * P.max_hop;
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= NP) return;
  const bool adjacent = p % P.max_hop == 0;
  double c;
  if (P.pair_status[p]) {
    c = adjacent ? (double)NAN : (double)INFINITY;
  } else {
    double trav = P.pair_trav[p];
    const double base = P.pair_effort[(int64_t)(P.order - 1) * NP + p] + P.w * P.pair_T[p];
    if (adjacent) {
      if (!isfinite(trav)) trav = 0.0;
      c = base + trav;
    } else {
      // (a timed shortcut, include/mplx_reserve_poly.h: ... and clear of the reservations, inside the table's horizon)
      const bool clear = !P.pair_hit || P.pair_hit[p] == -1;
      c = (P.pair_valid[p] == 1 && isfinite(trav) && clear) ? base + trav : (double)INFINITY;
    }
  }
  P.edge_cost[p] = c;
}

// shortcut_dp_kernel: one lane per query.  dist / pred live in scratch rows [w][Q]; every candidate is one add, ties go
// to the smallest i (the scan ascends and replaces on < only).
__global__ __launch_bounds__(kBlock) void shortcut_dp_kernel(const ShortcutArgs P) {
  const int64_t Q = P.n_query;
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= Q) return;
  const int wm = P.w_max, mh = P.max_hop;
  int W = P.n_wp ? P.n_wp[k] : wm;
  if (W > wm) W = wm;
  if (P.chain_hit) {  // a timed shortcut: the smallest conflict of the chain's own edges, else -2 past the horizon, else -1
    long long ch = -1;
    for (int i = 0; i + 1 < W; i++) {
      const long long h = P.pair_hit[(k * (wm - 1) + i) * mh];
      if (h >= 0 ? (ch < 0 || h < ch) : (h == -2 && ch == -1)) ch = h;
    }
    P.chain_hit[k] = ch;
  }
  for (int s = 0; s < wm - 1; s++) P.src_index[(int64_t)s * Q + k] = -1;
  if (P.keep)
    for (int w = 0; w < wm; w++) P.keep[(int64_t)w * P.keep_stride + k] = -1;
  if (W < 2) {
    if (P.status) P.status[k] = 1;  // MPLX_SOLVE_EMPTY
    if (P.n_keep) P.n_keep[k] = 0;
    if (P.cost) P.cost[k] = NAN;
    if (P.chain_cost) P.chain_cost[k] = NAN;
    return;
  }
  const double *c = P.edge_cost + k * (wm - 1) * mh;  // c[i][j] at c[i * mh + (j - i - 1)]
  bool bad = false;
  double chain = 0.0;
  for (int i = 0; i + 1 < W; i++) {
    const double e = c[(int64_t)i * mh];
    bad = bad || e != e;
    chain = chain + e;
  }
  P.dist[k] = 0.0;
  P.pred[k] = -1;
  for (int j = 1; j < W; j++) {
    double best = INFINITY;
    int bi = j - 1;
    for (int i = j - mh > 0 ? j - mh : 0; i < j; i++) {
      const double v = P.dist[(int64_t)i * Q + k] + c[(int64_t)i * mh + (j - i - 1)];
      if (v < best) {
        best = v;
        bi = i;
      }
    }
    if (bad) {  // the identity chain
      best = NAN;
      bi = j - 1;
    }
    P.dist[(int64_t)j * Q + k] = best;
    P.pred[(int64_t)j * Q + k] = bi;
  }
  int n = 1;
  for (int j = W - 1; j > 0; j = P.pred[(int64_t)j * Q + k]) n++;
  int pos = n - 1;
  for (int j = W - 1; j > 0;) {
    const int i = P.pred[(int64_t)j * Q + k];
    if (P.keep) P.keep[(int64_t)pos * P.keep_stride + k] = j;
    P.src_index[(int64_t)(pos - 1) * Q + k] = (int32_t)((k * (wm - 1) + i) * mh + (j - i - 1));
    pos--;
    j = i;
  }
  if (P.keep) P.keep[k] = 0;
  if (P.status) P.status[k] = bad ? 16 : 0;  // MPLX_SHORTCUT_BAD_CHAIN
  if (P.n_keep) P.n_keep[k] = n;
  if (P.cost) P.cost[k] = bad ? (double)NAN : P.dist[(int64_t)(W - 1) * Q + k];
  if (P.chain_cost) P.chain_cost[k] = bad ? (double)NAN : chain;
}

template <int D>
hipError_t limits_dim(const LimitsArgs &a, hipStream_t s) {
  const int64_t sb = (a.n_prob * a.s_max + kBlock - 1) / kBlock, nb = (a.n_prob + kBlock - 1) / kBlock;
  if (sb > 0x7fffffffLL) return hipErrorInvalidValue;
  if (a.all_roots)
    hipLaunchKernelGGL((poly_limits_kernel<D, true>), dim3((unsigned)sb), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((poly_limits_kernel<D, false>), dim3((unsigned)sb), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL((poly_limits_reduce_kernel<D>), dim3((unsigned)nb), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_poly_load(int dim, const PolyLoadArgs &a, hipStream_t s) {
  if (a.n_prob == 0) return hipSuccess;
  const int64_t blocks = (a.n_prob + kLoadBlock - 1) / kLoadBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (dim == 2) hipLaunchKernelGGL((poly_load_kernel<2>), dim3((unsigned)blocks), dim3(kLoadBlock), 0, s, a);
  else if (dim == 3) hipLaunchKernelGGL((poly_load_kernel<3>), dim3((unsigned)blocks), dim3(kLoadBlock), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_poly_limits(int dim, const LimitsArgs &a, hipStream_t s) {
  if (a.n_prob == 0 || a.s_max == 0) return hipSuccess;
  if (dim == 2) return limits_dim<2>(a, s);
  if (dim == 3) return limits_dim<3>(a, s);
  return hipErrorInvalidValue;
}

hipError_t launch_shortcut_pairs(int dim, const ShortcutArgs &a, hipStream_t s) {
  const int64_t np = a.n_query * (a.w_max - 1) * a.max_hop, blocks = (np + kBlock - 1) / kBlock;
  if (np == 0) return hipSuccess;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (dim == 2) hipLaunchKernelGGL((shortcut_pairs_kernel<2>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  else if (dim == 3) hipLaunchKernelGGL((shortcut_pairs_kernel<3>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_shortcut_dp(const ShortcutArgs &a, hipStream_t s) {
  const int64_t np = a.n_query * (a.w_max - 1) * a.max_hop, pb = (np + kBlock - 1) / kBlock, qb = (a.n_query + kBlock - 1) / kBlock;
  if (np == 0) return hipSuccess;
  if (pb > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(shortcut_cost_kernel, dim3((unsigned)pb), dim3(kBlock), 0, s, a);
  hipLaunchKernelGGL(shortcut_dp_kernel, dim3((unsigned)qb), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
