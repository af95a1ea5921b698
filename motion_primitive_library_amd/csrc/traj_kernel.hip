// traj_kernel.hip -- Trajectory<Dim> for gfx950 (MI355X): the chain of primitives behind K action sequences, its
// efforts, Command / Waypoint samples and env_map::traverse_trajectory on the map the context holds
// (include/mplx_traj.h; reference include/mpl_basis/trajectory.h, primitive.h:92-145, env_map.h:229-255).
//
// traj_chain_kernel<D, K>: one lane per trajectory, the shape of rollout_kernel.  The state stays in registers; a step
// is the successor evaluation of mplx_pair_device.h (dev::Ax<K>, the `0.0 +` forms; no validity check of any kind) and
// writes one row set of the segment table (TrajArgs, mplx_internal.h): coefficients c1 .. c5 per axis, the yaw
// primitive, tau.  The five efforts are summed per segment in the reference's order with its expression trees.
//
// traj_sample_kernel<D, FORM>: one lane per sample, consecutive lanes consecutive samples of one trajectory: the row
// stores are coalesced and a wave's segment rows are mostly one broadcast load.  The segment is a guess from tau / dt
// corrected against the stored taus until it is the reference's first match.
//
// traj_traverse_kernel<D, G>: G lanes of a wave per trajectory, rounds of G samples, as ray_kernel: the map bytes of a
// round are independent loads.  Ballots cut down to the group give the skip bit (compare with the neighbouring lane's
// index, lane 0 with the last index of the previous round), the first counted sample that ends the trajectory and the
// counts; the ordered sum walks the set bits of the round's `adds` ballot and broadcasts each term with __shfl: at
// most G adds per round, none on occupancy maps.  The loop bound is the n the chain launch left on the device.
//
// prior_sample_kernel<D> / prior_build_kernel<D>: the prior table of an open set (include/mplx_prior.h) on the same segment
// table, with find_segment / eval_segment as the kernels above use them; stated where they are defined, further down.
//
// Bit-exactness: -ffp-contract=off, true divisions, power by repeated multiply, sums in the reference's order.  The
// coefficient c0 of a forward primitive is 0: its terms of p / v / a / j are +0.0 for the finite tau >= 0 evaluated here
// and are stated as the leading `0.0 +`; the effort formulas keep c0 as a variable.
#include "mplx_internal.h"
#include "mplx_pair_device.h"
#include "mplx_scale_math.h"
#include "mplx_traj_device.h"

#include <math.h>

namespace mplx {
namespace {

using traj::Sample;
using traj::eval_segment;
using traj::find_segment;

constexpr int kBlock = 256;

// primitive.h:92-122 for one axis: J(t, order) with c[0] .. c[4] (c[5] does not enter); pN = t^N by repeated multiply
__device__ __forceinline__ double effort_1d(const double (&c)[5], double t, int order) {
  const double p2 = t * t, p3 = p2 * t, p4 = p3 * t, p5 = p4 * t, p6 = p5 * t, p7 = p6 * t, p8 = p7 * t, p9 = p8 * t;
  const double c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3], c4 = c[4];
  if (order == 1) {
    double j = c0 * c0 / 5184 * p9;
    j = j + c0 * c1 / 576 * p8;
    j = j + (c1 * c1 / 252 + c0 * c2 / 168) * p7;
    j = j + (c0 * c3 / 72 + c1 * c2 / 36) * p6;
    j = j + ((c2 * c2 / 20 + c0 * c4 / 60) + c1 * c3 / 15) * p5;
    j = j + (c2 * c3 / 4 + c1 * c4 / 12) * p4;
    j = j + (c3 * c3 / 3 + c2 * c4 / 3) * p3;
    j = j + c3 * c4 * t * t;
    return j + c4 * c4 * t;
  }
  if (order == 2) {
    double j = c0 * c0 / 252 * p7;
    j = j + c0 * c1 / 36 * p6;
    j = j + (c1 * c1 / 20 + c0 * c2 / 15) * p5;
    j = j + (c0 * c3 / 12 + c1 * c2 / 4) * p4;
    j = j + (c2 * c2 / 3 + c1 * c3 / 3) * p3;
    j = j + c2 * c3 * t * t;
    return j + c3 * c3 * t;
  }
  if (order == 3) {
    double j = c0 * c0 / 20 * p5;
    j = j + c0 * c1 / 4 * p4;
    j = j + (c1 * c1 + c0 * c2) / 3 * p3;
    j = j + c1 * c2 * t * t;
    return j + c2 * c2 * t;
  }
  double j = c0 * c0 / 3 * p3;
  j = j + c0 * c1 * t * t;
  return j + c1 * c1 * t;
}

template <int D, int K>
__global__ __launch_bounds__(kBlock) void traj_chain_kernel(const TrajArgs R) {
  const ExpandArgs &A = R.env;
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= R.n_traj) return;
  const int64_t N = R.n_traj;
  constexpr int F = 4 * D + 2, NC = 5 * D + 2;
  double s[F];
  {
    const double *sp = R.starts + (R.n_starts == 1 ? 0 : k);
#pragma unroll
    for (int f = 0; f < F; f++) s[f] = sp[f * R.start_stride];
  }
  const double T = A.dt;
  double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double tau = 0.0;
  uint8_t status = 0;
  int S = 0;
  for (int h = 0; h < R.horizon; h++) {
    const int a = R.actions[(int64_t)h * R.action_stride + k];
    if (a == -1) break;
    if (a < -1 || a >= A.nU) {
      status = 2;  // MPLX_TRAJ_BAD_ACTION: the control table is never read out of range
      break;
    }
    const double *up = A.U + (int64_t)a * A.udim;
    const double uy = R.yaw ? up[D] : 0.0, cyaw = R.yaw ? s[4 * D] : 0.0;  // (no yaw bit: pr_yaw_ stays all zero)
    dev::Ax<K> ax[D];
    R.tab_tau[(int64_t)h * N + k] = tau;
    traj::chain_segment<D, K>(s, up, uy, cyaw, ax, R.tab_seg + (int64_t)h * NC * N + k, N);
    if (R.seg_state) {
      double *o = R.seg_state + (int64_t)h * R.seg_stride + k;
#pragma unroll
      for (int f = 0; f < F; f++) o[(int64_t)f * (R.horizon + 1) * R.seg_stride] = s[f];
    }
    if (R.effort) {
      // Trajectory::J: j = 0; j += seg.J(c).  Primitive::J: j = 0; j += pr.J(t, c) in axis order.
#pragma unroll
      for (int o = 1; o <= 4; o++) {
        double j = 0.0;
#pragma unroll
        for (int i = 0; i < D; i++) {
          const double c[5] = {0.0, ax[i].c1, ax[i].c2, ax[i].c3, ax[i].c4};
          j = j + effort_1d(c, T, o);
        }
        e[o - 1] = e[o - 1] + j;
      }
      const double cy[5] = {0.0, 0.0, 0.0, 0.0, uy};
      e[4] = e[4] + effort_1d(cy, T, 1);
    }
    // s_{h+1} = pr.evaluate(dt) (primitive.h:321-331), t + dt (env_map.h:161)
#pragma unroll
    for (int i = 0; i < D; i++) {
      s[i] = ax[i].template pos<true>(T);
      s[D + i] = ax[i].template vel<true>(T);
      s[2 * D + i] = ax[i].template acc<true>(T);
      s[3 * D + i] = ax[i].template jrk<true>(T);
    }
    s[4 * D] = R.yaw ? dev::wrap_angle((0.0 + uy * T) + cyaw) : 0.0;
    s[4 * D + 1] = s[4 * D + 1] + T;
    tau = T + tau;  // trajectory.h:54
    S++;
  }
  R.tab_tau[(int64_t)S * N + k] = tau;
  if (R.seg_state) {
    double *o = R.seg_state + (int64_t)S * R.seg_stride + k;
#pragma unroll
    for (int f = 0; f < F; f++) o[(int64_t)f * (R.horizon + 1) * R.seg_stride] = s[f];
  }
  if (S == 0) status |= 1;  // MPLX_TRAJ_EMPTY
  // env_map.h:231: n = ceil(v_max * T / res); -1 where the conversion to int is not defined
  const double cn = ceil(A.v_max * tau / A.res);
  const int n = !(cn < 2147483648.0) ? -1 : cn > 0.0 ? (int)cn : 0;
  R.tab_S[k] = S;
  R.tab_n[k] = n;
  R.tab_status[k] = status;
  R.tab_T[k] = tau;
  if (R.status) R.status[k] = status;
  if (R.n_segs) R.n_segs[k] = S;
  if (R.total_time) R.total_time[k] = tau;
  if (R.effort) {
#pragma unroll
    for (int o = 0; o < 5; o++) R.effort[(int64_t)o * R.effort_stride + k] = e[o];
  }
}

// LAMBDA (a solved set that holds a Lambda, include/mplx_scale.h): the time is real time, tau = getTau(time) under the
// Lambda's mode; a problem without one (lam_n == 0) is sampled as ever.
template <int D, int FORM, bool POLY = false, bool LAMBDA = false>
__global__ __launch_bounds__(kBlock) void traj_sample_kernel(const TrajArgs R) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t N = R.n_traj;
  if (g >= N * R.count) return;
  const int64_t k = g / R.count, i = g - k * R.count;
  const int S = R.tab_S[k];
  if (S == 0) return;
  const double T = R.tab_T[k];
  const int nl = LAMBDA ? R.lam_n[k] : 0;
  double time;
  if (R.n_uniform > 0) {
    const double total = nl > 0 ? R.lam_total[k] : T;
    const double step = total / (double)R.n_uniform;  // trajectory.h:233-234
    time = LAMBDA ? scale::uniform_time(i, R.n_uniform, step, total, nl > 0 && R.lam == 2) : (double)i * step;
  } else {
    time = R.times[k * R.time_stride + i];
  }
  constexpr int kRows = FORM == 0 ? 4 * D + 3 : 4 * D + 1;
  double *o = R.out + k * R.sample_stride + i;
  if (!isfinite(time)) {
#pragma unroll
    for (int r = 0; r < kRows; r++) o[(int64_t)r * R.row_stride] = NAN;
    return;
  }
  double tau = time, lambda = 1.0, lambda_dot = 0.0;
  if (nl > 0) {
    const scale::TableLoader ld{R.lam_seg + k, N};
    double raw;
    bool found;
    tau = scale::sample_tau(ld, nl, R.lam == 2, time, R.lam_total[k], T, &raw, &found, &lambda, &lambda_dot);
  } else {
    if (tau < 0) tau = 0;
    if (tau > T) tau = T;
  }
  const double *taus = R.tab_tau + k;
  const int id = find_segment<FORM == 0, POLY>(taus, N, S, tau, R.env.dt);
  tau -= taus[(int64_t)id * N];
  Sample<D> sm;
  eval_segment<D, FORM == 0, true, POLY>(R.tab_seg + (int64_t)id * ((POLY ? 6 : 5) * D + 2) * N + k, N, tau, sm, lambda, lambda_dot);
#pragma unroll
  for (int d = 0; d < D; d++) {
    o[(int64_t)(0 * D + d) * R.row_stride] = sm.pos[d];
    o[(int64_t)(1 * D + d) * R.row_stride] = sm.vel[d];
    o[(int64_t)(2 * D + d) * R.row_stride] = sm.acc[d];
    o[(int64_t)(3 * D + d) * R.row_stride] = sm.jrk[d];
  }
  o[(int64_t)(4 * D) * R.row_stride] = sm.yaw;
  if (FORM == 0) {
    o[(int64_t)(4 * D + 1) * R.row_stride] = sm.yaw_dot;
    o[(int64_t)(4 * D + 2) * R.row_stride] = time;
  }
}

template <int D, int G, bool POLY = false>
__global__ __launch_bounds__(kBlock) void traj_traverse_kernel(const TrajArgs R) {
  const ExpandArgs &A = R.env;
  constexpr int kTraj = kBlock / G;
  const int64_t N = R.n_traj;
  const int64_t k = (int64_t)blockIdx.x * kTraj + threadIdx.x / G;
  const bool have = k < N;
  const int lane = threadIdx.x & 63;
  const int gl = lane & (G - 1), gbase = lane & ~(G - 1);
  const uint64_t group_bits = G == 64 ? ~0ull : ((1ull << G) - 1);
  const int32_t mdim[3] = {A.dim0, A.dim1, A.dim2};
  const double org[3] = {A.org0, A.org1, A.org2};

  const int S = have ? R.tab_S[k] : 0;
  const double T = have ? R.tab_T[k] : 0.0;
  int n = 0;
  if (POLY) {  // a solved set outlives parameter changes: n of env_map.h:231 from the v_max and res of now
    if (S > 0) {
      const double cn = ceil(A.v_max * T / A.res);
      n = !(cn < 2147483648.0) ? -1 : cn > 0.0 ? (int)cn : 0;
    }
  } else if (have) {
    n = R.tab_n[k];
  }
  const bool active = have && S > 0 && n >= 0;
  const double step = T / (double)n;  // trajectory.h:233
  const double *taus = R.tab_tau + (have ? k : 0);
  const bool pot = A.pot != nullptr;

  double cost = 0.0;
  int n_cells = 0, stop = -1;
  int carry = -1;  // env_map.h:234: prev_idx
  int64_t i = gl;  // this lane's sample of the round
  bool done = !active;
  while (__ballot(!done) != 0ull) {
    const bool has = !done && i <= (int64_t)n;
    int idx = 0;
    bool inside = false;
    double term = 0.0;
    int v = 0;
    if (has) {
      double tau = (double)i * step;  // >= 0 and finite
      if (tau > T) tau = T;
      const int id = find_segment<true, POLY>(taus, N, S, tau, A.dt);
      tau -= taus[(int64_t)id * N];
      Sample<D> sm;
      eval_segment<D, true, false, POLY>(R.tab_seg + (int64_t)id * ((POLY ? 6 : 5) * D + 2) * N + k, N, tau, sm);
      uint32_t ui = 0, mul = 1;
      inside = true;
#pragma unroll
      for (int d = 0; d < D; d++) {
        // map_util.h:103-108; a value the reference could not convert saturates (NaN: the lower end)
        double c = round((sm.pos[d] - org[d]) / A.res - 0.5);
        c = fmin(fmax(c, -2147483648.0), 2147483647.0);
        const int ci = (int)c;
        inside = inside && ci >= 0 && ci < mdim[d];
        ui += (uint32_t)ci * mul;  // map_util.h:34-41 in wrapping 32-bit arithmetic, also for cells outside
        mul *= (uint32_t)mdim[d];
      }
      idx = (int)ui;
      if (inside) v = pot ? A.pot[idx] : A.map[idx];
      if (pot) {
        double q = 0;
#pragma unroll
        for (int d = 0; d < D; d++) q += sm.vel[d] * sm.vel[d];
        term = A.pot_w * v + A.grad_w * sqrt(q);  // env_map.h:246-247
      }
    }
    int prev = __shfl_up(idx, 1);
    if (gl == 0) prev = carry;
    const bool counted = has && idx != prev;  // env_map.h:238: the skip comes before every other question
    const bool ends = counted && (!inside || (pot ? v >= 100 : v == 100));
    const uint64_t end_b = (__ballot(ends) >> gbase) & group_bits;
    const int first_end = end_b ? __builtin_ctzll(end_b) : G;
    const uint64_t cnt_b = (__ballot(counted && gl <= first_end) >> gbase) & group_bits;
    uint64_t add_b = (__ballot(counted && gl < first_end && pot && v > 0 && v < 100) >> gbase) & group_bits;
    n_cells += __popcll(cnt_b);
    // the ordered sum: one IEEE add per adding sample, in sample order
    while (__ballot(add_b != 0ull) != 0ull) {
      const int b = add_b ? __builtin_ctzll(add_b) : 0;
      const double tv = __shfl(term, gbase + b);
      if (add_b) {
        cost = cost + tv;
        add_b &= add_b - 1;
      }
    }
    carry = __shfl(idx, gbase + G - 1);
    if (end_b && !done) {
      stop = (int)(i - gl) + first_end;
      cost = INFINITY;
      done = true;
    }
    i += G;
    if (i - gl > (int64_t)n) done = true;  // the next round's first sample is past the last one
  }
  if (!have || gl != 0) return;
  const uint8_t status = (uint8_t)(R.tab_status[k] | (n < 0 ? 4 : 0));  // MPLX_TRAJ_BAD
  if (R.status) R.status[k] = status;
  if (R.cost) R.cost[k] = n < 0 ? (double)NAN : cost;
  if (R.n_samples) R.n_samples[k] = active ? n + 1 : 0;
  if (R.n_cells) R.n_cells[k] = n_cells;
  if (R.stop_sample) R.stop_sample[k] = stop;
}

// ---- the prior table of an open set (include/mplx_prior.h; env_map.h:189-226 as csrc/host_planner.hpp restates it) ----
//
// prior_sample_kernel<D>: one lane per sample of the traversal (the samples traj_traverse_kernel walks, the same
// expressions): its cell index and its term potential_weight * value + gradient_weight * |vel| -- the map bytes of a wave
// are independent loads.  A sample outside the map reads 0; no range test on the value (env_map.h:205-211).
// prior_build_kernel<D>: one lane per trajectory: the two serial chains (t_k by sequential addition; the prefix of the
// terms in sample order, one IEEE add each), pos / togo, and the goal the query's pushes use from now on.  Every loop is
// bounded by s_cap / k_cap, the host's bounds; a trajectory that would pass them is MPLX_TRAJ_BAD.
template <int D>
__global__ __launch_bounds__(kBlock) void prior_sample_kernel(const PriorArgs P) {
  const TrajArgs &R = P.traj;
  const ExpandArgs &A = R.env;
  const int64_t N = R.n_traj;
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= N * P.s_cap) return;
  const int64_t k = g / P.s_cap, i = g - k * P.s_cap;
  const int S = R.tab_S[k], n = R.tab_n[k];
  if (S <= 0 || n < 1 || (int64_t)n + 1 > P.s_cap || i > (int64_t)n) return;
  const double T = R.tab_T[k];
  const double step = T / (double)n;  // trajectory.h:233
  const double *taus = R.tab_tau + k;
  double tau = (double)i * step;  // >= 0 and finite
  if (tau > T) tau = T;
  const int id = find_segment<true>(taus, N, S, tau, A.dt);
  tau -= taus[(int64_t)id * N];
  Sample<D> sm;
  eval_segment<D, true, false>(R.tab_seg + (int64_t)id * (5 * D + 2) * N + k, N, tau, sm);
  const int32_t mdim[3] = {A.dim0, A.dim1, A.dim2};
  const double org[3] = {A.org0, A.org1, A.org2};
  uint32_t ui = 0, mul = 1;
  bool inside = true;
#pragma unroll
  for (int d = 0; d < D; d++) {
    // map_util.h:103-108; a value the reference could not convert saturates (NaN: the lower end)
    double c = round((sm.pos[d] - org[d]) / A.res - 0.5);
    c = fmin(fmax(c, -2147483648.0), 2147483647.0);
    const int ci = (int)c;
    inside = inside && ci >= 0 && ci < mdim[d];
    ui += (uint32_t)ci * mul;  // map_util.h:34-41 in wrapping 32-bit arithmetic, also for cells outside
    mul *= (uint32_t)mdim[d];
  }
  const int idx = (int)ui;
  double term = 0.0;
  if (A.pot) {
    const int v = inside ? A.pot[idx] : 0;
    double q = 0;
#pragma unroll
    for (int d = 0; d < D; d++) q += sm.vel[d] * sm.vel[d];
    term = A.pot_w * v + A.grad_w * sqrt(q);  // env_map.h:209-210
  }
  P.s_idx[k * P.s_cap + i] = idx;
  P.s_term[k * P.s_cap + i] = term;
}

// waypoint.h:93-125 with the control flag at run time (the prior's), as host::lattice_hash states it
template <int D>
__device__ __forceinline__ uint64_t prior_goal_hash(int control, const Sample<D> &sm) {
  uint64_t h = 0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    if (control & 1) dev::fold(h, pair::quantise(sm.pos[i], 0.01));
    if (control & 2) dev::fold(h, pair::quantise(sm.vel[i], 0.1));
    if (control & 4) dev::fold(h, pair::quantise(sm.acc[i], 0.1));
    if (control & 8) dev::fold(h, pair::quantise(sm.jrk[i], 0.1));
  }
  if (control & 16) dev::fold(h, pair::quantise(sm.yaw, 0.1));
  return h;
}

template <int D>
__global__ __launch_bounds__(kBlock) void prior_build_kernel(const PriorArgs P, int control) {
  const TrajArgs &R = P.traj;
  const ExpandArgs &A = R.env;
  const int64_t N = R.n_traj;
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= N) return;
  const int S = R.tab_S[k], n = R.tab_n[k];
  const double T = R.tab_T[k];
  const double *taus = R.tab_tau + k;
  uint8_t status = R.tab_status[k];
  if (n < 0 || (int64_t)n + 1 > P.s_cap) status |= 4;  // MPLX_TRAJ_BAD
  int64_t cnt = 0;
  if (S > 0 && !(status & 4)) {
    const double total = P.traverse[k] + A.w * T;  // env_map.h:194
    const double step = T / (double)n;
    double *costs = P.costs + k * P.k_cap;
    const int32_t *s_idx = P.s_idx + k * P.s_cap;
    const double *s_term = P.s_term + k * P.s_cap;
    const bool pot = A.pot != nullptr && n >= 1;
    // env_map.h:197-216: the loop over samples of step k is a prefix of the loop of step k + 1 -- the same adds in the
    // same order, carried on
    double t = 0.0, pc = 0.0;
    int64_t j = 0;
    int prev = -1;
    for (; cnt < P.k_cap && t < T; cnt++) {
      if (pot) {
        while (j <= (int64_t)n) {  // (n + 1 <= s_cap)
          if ((double)j * step >= t) break;
          const int idx = s_idx[j];
          if (idx != prev) {
            prev = idx;
            pc = pc + s_term[j];
          }
          j++;
        }
      }
      costs[cnt] = A.w * t + pc;
      t = t + P.dt;
    }
    if (t < T) {  // (more steps than the host's bound: never with finite dt)
      status |= 4;
      cnt = 0;
    }
    t = 0.0;
    for (int64_t kk = 0; kk < cnt; kk++) {
      int64_t id = (int64_t)(int)(t / P.dt);  // env_map.h:219: the truncated quotient
      id = id < 0 ? 0 : (id < cnt ? id : cnt - 1);
      double tau = t;
      if (tau > T) tau = T;
      const int seg = find_segment<false>(taus, N, S, tau, A.dt);
      tau -= taus[(int64_t)seg * N];
      Sample<D> sm;
      eval_segment<D, false, false>(R.tab_seg + (int64_t)seg * (5 * D + 2) * N + k, N, tau, sm);
#pragma unroll
      for (int d = 0; d < D; d++) P.pos[(k * P.k_cap + kk) * D + d] = sm.pos[d];
      P.togo[k * P.k_cap + kk] = total - costs[id];
      t = t + P.dt;
    }
  }
  P.n_steps[k] = (int32_t)cnt;
  P.status[k] = status;
  // the goal of query k from now on: the prior's end (env_map.h:225), or what mplx_open_set_goals gave
  PostFuse G = P.goals0[k];
  if (cnt > 0) {
    Sample<D> sm;
    eval_segment<D, false, true>(R.tab_seg + (int64_t)(S - 1) * (5 * D + 2) * N + k, N, T - taus[(int64_t)(S - 1) * N], sm);
#pragma unroll
    for (int d = 0; d < D; d++) {
      G.goal[d] = sm.pos[d];
      G.goal[D + d] = sm.vel[d];
      G.goal[2 * D + d] = sm.acc[d];
      G.goal[3 * D + d] = sm.jrk[d];
    }
    G.goal[4 * D] = sm.yaw;
    G.goal[4 * D + 1] = 0.0;  // (Trajectory::evaluate returns a fresh Waypoint: t = 0)
    G.goal_hash = prior_goal_hash<D>(control, sm);
  }
  P.goals[k] = G;
#pragma unroll
  for (int f = 0; f < 14; f++) P.goal_row[k * 14 + f] = G.goal[f];
  P.goal_hash[k] = G.goal_hash;
}

template <int D, int K>
hipError_t chain_one(const TrajArgs &a, hipStream_t s) {
  const int64_t blocks = (a.n_traj + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((traj_chain_kernel<D, K>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <int D>
hipError_t chain_dim(int control, const TrajArgs &a, hipStream_t s) {
  switch (control & 0x0f) {
    case 0x01: return chain_one<D, 1>(a, s);
    case 0x03: return chain_one<D, 2>(a, s);
    case 0x07: return chain_one<D, 3>(a, s);
    case 0x0f: return chain_one<D, 4>(a, s);
    default: return hipErrorInvalidValue;
  }
}

template <int D, int FORM>
hipError_t sample_one(const TrajArgs &a, hipStream_t s) {
  const int64_t blocks = (a.n_traj * a.count + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (a.poly && a.lam)
    hipLaunchKernelGGL((traj_sample_kernel<D, FORM, true, true>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  else if (a.poly)
    hipLaunchKernelGGL((traj_sample_kernel<D, FORM, true>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((traj_sample_kernel<D, FORM>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <int D, int G>
hipError_t traverse_one(const TrajArgs &a, hipStream_t s) {
  const int64_t blocks = (a.n_traj + kBlock / G - 1) / (kBlock / G);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (a.poly)
    hipLaunchKernelGGL((traj_traverse_kernel<D, G, true>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  else
    hipLaunchKernelGGL((traj_traverse_kernel<D, G>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

// Efforts and waypoints of a solved set (include/mplx_solve.h): one lane per problem over its stored segments.
// Trajectory::J / Primitive::J as traj_chain_kernel sums them, with the segment's own duration and all of c0 .. c4.
template <int D>
__global__ __launch_bounds__(kBlock) void poly_info_kernel(const TrajArgs R) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= R.n_traj) return;
  const int64_t N = R.n_traj;  // (the stride of the table)
  constexpr int F = 4 * D + 2, NC = 6 * D + 2;
  const int S = R.tab_S[k];
  if (R.status) R.status[k] = R.tab_status[k];
  if (S == 0) return;  // a failed problem: its status only
  if (R.n_segs) R.n_segs[k] = S;
  if (R.total_time) R.total_time[k] = R.tab_T[k];
  if (R.effort) {
    double e[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < S; s++) {
      const double *seg = R.tab_seg + (int64_t)s * NC * N + k;
      const double T = R.tab_dt[(int64_t)s * N + k];
#pragma unroll
      for (int o = 1; o <= 4; o++) {
        double j = 0.0;
#pragma unroll
        for (int i = 0; i < D; i++) {
          const double c[5] = {seg[(6 * i + 0) * N], seg[(6 * i + 1) * N], seg[(6 * i + 2) * N], seg[(6 * i + 3) * N],
                               seg[(6 * i + 4) * N]};
          j = j + effort_1d(c, T, o);
        }
        e[o - 1] = e[o - 1] + j;
      }
      const double cy[5] = {0.0, 0.0, 0.0, 0.0, seg[(6 * D) * N]};
      e[4] = e[4] + effort_1d(cy, T, 1);
    }
#pragma unroll
    for (int o = 0; o < 5; o++) R.effort[(int64_t)o * R.effort_stride + k] = e[o];
  }
  if (R.seg_state) {
    const int64_t W1 = (int64_t)R.horizon + 1;
    for (int w = 0; w <= S; w++) {
#pragma unroll
      for (int f = 0; f < F; f++) R.seg_state[(f * W1 + w) * R.seg_stride + k] = R.tab_wp[(f * W1 + w) * N + k];
    }
  }
}

}  // namespace

hipError_t launch_traj_chain(int dim, int control, const TrajArgs &a, hipStream_t s) {
  if (a.n_traj == 0) return hipSuccess;
  if (dim == 2) return chain_dim<2>(control, a, s);
  if (dim == 3) return chain_dim<3>(control, a, s);
  return hipErrorInvalidValue;
}

hipError_t launch_traj_sample(int dim, int form, const TrajArgs &a, hipStream_t s) {
  if (a.n_traj * a.count == 0) return hipSuccess;
  if (dim == 2) return form == 0 ? sample_one<2, 0>(a, s) : sample_one<2, 1>(a, s);
  if (dim == 3) return form == 0 ? sample_one<3, 0>(a, s) : sample_one<3, 1>(a, s);
  return hipErrorInvalidValue;
}

hipError_t launch_poly_info(int dim, const TrajArgs &a, hipStream_t s) {
  if (a.n_traj == 0) return hipSuccess;
  const int64_t blocks = (a.n_traj + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (dim == 2) hipLaunchKernelGGL((poly_info_kernel<2>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  else if (dim == 3) hipLaunchKernelGGL((poly_info_kernel<3>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_prior_build(int dim, int control, const PriorArgs &a, hipStream_t s) {
  const int64_t N = a.traj.n_traj;
  if (N <= 0) return hipSuccess;
  if (dim != 2 && dim != 3) return hipErrorInvalidValue;
  const int64_t sb = (N * a.s_cap + kBlock - 1) / kBlock, nb = (N + kBlock - 1) / kBlock;
  if (sb > 0x7fffffffLL) return hipErrorInvalidValue;
  if (dim == 2) {
    hipLaunchKernelGGL((prior_sample_kernel<2>), dim3((unsigned)sb), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL((prior_build_kernel<2>), dim3((unsigned)nb), dim3(kBlock), 0, s, a, control);
  } else {
    hipLaunchKernelGGL((prior_sample_kernel<3>), dim3((unsigned)sb), dim3(kBlock), 0, s, a);
    hipLaunchKernelGGL((prior_build_kernel<3>), dim3((unsigned)nb), dim3(kBlock), 0, s, a, control);
  }
  return hipGetLastError();
}

hipError_t launch_traj_traverse(int dim, int lanes, const TrajArgs &a, hipStream_t s) {
  if (a.n_traj == 0) return hipSuccess;
  if (dim == 2) {
    if (lanes == 4) return traverse_one<2, 4>(a, s);
    if (lanes == 16) return traverse_one<2, 16>(a, s);
    if (lanes == 64) return traverse_one<2, 64>(a, s);
  } else if (dim == 3) {
    if (lanes == 4) return traverse_one<3, 4>(a, s);
    if (lanes == 16) return traverse_one<3, 16>(a, s);
    if (lanes == 64) return traverse_one<3, 64>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace mplx
