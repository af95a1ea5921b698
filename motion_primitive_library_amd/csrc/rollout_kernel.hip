// rollout_kernel.hip -- batched rollouts for gfx950 (MI355X): cost and validity of K action sequences on the map the
// context holds (include/mplx_rollout.h).
//
// One lane walks one rollout, a wavefront 64 consecutive ones.  The state (4D+2 doubles) stays in registers from step
// to step; per step a wave reads one 256-byte segment of the step-major action array and gathers its 64 controls from
// a copy of the control table in LDS (global reads when the table is larger than kRolloutLdsControls).  With one
// shared start state the start is a broadcast load.  Every output is a [n_rollouts] row, written coalesced once.
//
// A step evaluates ONE (state, control) pair with the functions of mplx_pair_device.h -- the arithmetic of
// expand_kernel.hip, under the same bit-exactness rules (-ffp-contract=off, true divisions, t += dt, the leading
// `0.0 +`).  The prefix cost is ((0.0 + c_0) + c_1) + ..., one IEEE add per step in step order: the order in which A*
// forms g (reference include/mpl_planner/common/graph_search.h:107).
//
// Lanes stop at different steps and their sample loops differ in length; lanes are not re-packed.  A wave leaves the
// step loop as soon as none of its lanes is alive.
#include "mplx_internal.h"
#include "mplx_pair_device.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kBlock = 256;

template <int D, int K, bool YAW>
__global__ __launch_bounds__(kBlock) void rollout_kernel(const RolloutArgs R) {
  extern __shared__ double s_U[];
  const ExpandArgs &A = R.env;
  if (R.u_lds) {
    const int n = A.nU * A.udim;
    for (int i = threadIdx.x; i < n; i += kBlock) s_U[i] = A.U[i];
    __syncthreads();
  }
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool mine = k < R.n_rollouts;  // (lanes past the end stay for the barrier above and the ballots below)
  bool alive = mine;

  constexpr int F = 4 * D + 2;
  double s[F];  // pos, vel, acc, jrk, yaw, t: the Waypoint rows of include/mplx.h
#pragma unroll
  for (int f = 0; f < F; f++) s[f] = 0.0;
  if (mine) {
    const double *sp = R.starts + (R.n_starts == 1 ? 0 : k);
#pragma unroll
    for (int f = 0; f < F; f++) s[f] = sp[f * R.start_stride];
  }

  uint8_t status = 1;  // MPLX_SLOT_FINITE: complete unless a step says otherwise
  int steps = 0;
  double prefix = 0.0;
  bool amb = false;
  const bool heading = YAW && A.yaw_max > 0;
  const double cos_lim = heading ? cos(A.yaw_max) : 0.0;

  for (int h = 0; h < R.horizon; h++) {
    int a = -1;
    if (alive) a = R.actions[(int64_t)h * R.action_stride + k];
    if (alive && a == -1) {
      alive = false;  // the sequence ends here: complete
    } else if (alive && (a < -1 || a >= A.nU)) {
      status = 4;  // MPLX_ROLLOUT_BAD_ACTION: the control table is never read out of range
      alive = false;
    }
    if (__ballot(alive) == 0ull) break;
    if (alive) {
      double u[D], uy = 0.0;
      if (R.u_lds) {
        const double *up = s_U + a * A.udim;
#pragma unroll
        for (int i = 0; i < D; i++) u[i] = up[i];
        if (YAW) uy = up[D];
      } else {
        const double *up = A.U + (int64_t)a * A.udim;
#pragma unroll
        for (int i = 0; i < D; i++) u[i] = up[i];
        if (YAW) uy = up[D];
      }
      pair::Pair<D, K, YAW> P;
#pragma unroll
      for (int i = 0; i < D; i++) {
        // (rows the control order does not read: 0.0, as the dense kernel loads them)
        P.cpos[i] = s[0 * D + i];
        P.cvel[i] = (K >= 2) ? s[1 * D + i] : 0.0;
        P.cacc[i] = (K >= 3) ? s[2 * D + i] : 0.0;
        P.cjrk[i] = (K >= 4) ? s[3 * D + i] : 0.0;
      }
      P.cyaw = YAW ? s[4 * D] : 0.0;
      P.init(u, uy, A.dt);
      bool valid = true;
      // device trig; a decision inside the band is reported, not overridden (include/mplx_rollout.h)
      if (heading) valid = P.heading_valid(nullptr, 0, cos_lim, A.yaw.margin, A.yaw.tie_yaw, &amb);
      valid = P.limits_valid(A, valid);
      uint8_t st;
      double cost;
      int iters;
      P.classify(A, valid, &st, &cost, &iters);
      if (st == 1) {
        prefix = prefix + cost;
#pragma unroll
        for (int i = 0; i < D; i++) {
          s[0 * D + i] = P.npos[i];
          s[1 * D + i] = P.nvel[i];
          s[2 * D + i] = P.nacc[i];
          s[3 * D + i] = P.njrk[i];
        }
        s[4 * D] = P.nyaw;
        s[4 * D + 1] = s[4 * D + 1] + A.dt;  // env_map.h:161
        steps++;
      } else {
        status = st;
        alive = false;
      }
    }
  }
  if (!mine) return;

  if (R.status) R.status[k] = (amb && R.band) ? (uint8_t)(status | 0x80) : status;
  if (R.steps) R.steps[k] = steps;
  if (R.cost) R.cost[k] = status == 1 ? prefix : INFINITY;
  if (R.prefix_cost) R.prefix_cost[k] = prefix;
  if (R.end_state) {
    double *o = R.end_state + k;
#pragma unroll
    for (int f = 0; f < F; f++) o[f * R.end_stride] = s[f];
  }
  if (R.end_hash || R.post.heur || R.post.flags) {
    const uint64_t hash = pair::lattice_hash<D, K, YAW>(s, s + D, s + 2 * D, s + 3 * D, s[4 * D]);
    if (R.end_hash) R.end_hash[k] = hash;
    if (R.post.heur || R.post.flags) {
      MPLX_POST_GOAL(PG, R.post, D)
      double heur;
      unsigned int flags;
      dev::post_eval<D>(PG, hash, s, s + D, s + 2 * D, s[4 * D], &heur, &flags);
      if (R.post.heur) R.post.heur[k] = heur;
      if (R.post.flags) R.post.flags[k] = (uint8_t)flags;
    }
  }
}

template <int D, int K, bool YAW>
hipError_t launch_one(const RolloutArgs &a, hipStream_t stream) {
  if (a.n_rollouts == 0) return hipSuccess;
  const int64_t blocks = (a.n_rollouts + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds = a.u_lds ? (size_t)a.env.nU * a.env.udim * sizeof(double) : 0;
  hipLaunchKernelGGL((rollout_kernel<D, K, YAW>), dim3((unsigned)blocks), dim3(kBlock), lds, stream, a);
  return hipGetLastError();
}

template <int D>
hipError_t launch_dim(int control, const RolloutArgs &a, hipStream_t s) {
  switch (control) {
    case 0x01: return launch_one<D, 1, false>(a, s);
    case 0x03: return launch_one<D, 2, false>(a, s);
    case 0x07: return launch_one<D, 3, false>(a, s);
    case 0x0f: return launch_one<D, 4, false>(a, s);
    case 0x11: return launch_one<D, 1, true>(a, s);
    case 0x13: return launch_one<D, 2, true>(a, s);
    case 0x17: return launch_one<D, 3, true>(a, s);
    case 0x1f: return launch_one<D, 4, true>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t launch_rollout(int dim, int control, const RolloutArgs &args, hipStream_t stream) {
  if (dim == 2) return launch_dim<2>(control, args, stream);
  if (dim == 3) return launch_dim<3>(control, args, stream);
  return hipErrorInvalidValue;
}

}  // namespace mplx
