// wait_kernel.hip -- wait edges for gfx950 (MI355X): the zero control's entry appended to the successor lists of an
// expansion (include/mplx_wait.h states the semantics; tests/wait_model.py restates them sequentially).
//
// lists_add_wait_kernel<D, K, YAW>: one lane per list row, a workgroup 256 consecutive rows.  The lane loads its
// parent's state (coalesced: the frontier is field-major), evaluates the ONE pair (parent, U[a0]) with the functions of
// mplx_pair_device.h -- the arithmetic of expand_kernel.hip under the same bit-exactness rules (-ffp-contract=off, true
// divisions, the leading `0.0 +`) --, and where the row is eligible writes the entry behind the row's list and raises its
// count.  No map cell is read: an eligible pair does not move (env_map.h:163).  Every output of a row is written by the
// lane that owns it; the only atomic is the wave's sum into *n_added.  No LDS, no loop but the unrolled ones over D.
#include "mplx_internal.h"
#include "mplx_pair_device.h"

#include <math.h>

namespace mplx {
namespace {

constexpr int kBlock = 256;

template <int D, int K, bool YAW>
__global__ __launch_bounds__(kBlock) void lists_add_wait_kernel(const WaitArgs W) {
  const ExpandArgs &A = W.env;
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool added = false;
  if (k < W.n_rows && (W.parent_id == nullptr || W.parent_id[k] >= 0)) {
    constexpr int F = 4 * D + 2;
    const double *sp = W.parent_state + k;
    pair::Pair<D, K, YAW> P;
#pragma unroll
    for (int i = 0; i < D; i++) {
      // (rows the control order does not read: 0.0, as the dense kernel loads them)
      P.cpos[i] = sp[(int64_t)(0 * D + i) * W.parent_stride];
      P.cvel[i] = (K >= 2) ? sp[(int64_t)(1 * D + i) * W.parent_stride] : 0.0;
      P.cacc[i] = (K >= 3) ? sp[(int64_t)(2 * D + i) * W.parent_stride] : 0.0;
      P.cjrk[i] = (K >= 4) ? sp[(int64_t)(3 * D + i) * W.parent_stride] : 0.0;
    }
    P.cyaw = YAW ? sp[(int64_t)(4 * D) * W.parent_stride] : 0.0;
    const double tp = sp[(int64_t)(F - 1) * W.parent_stride];
    const double *up = A.U + (int64_t)W.a0 * A.udim;
    double u[D];
#pragma unroll
    for (int i = 0; i < D; i++) u[i] = up[i];
    P.init(u, YAW ? up[D] : 0.0, A.dt);
    bool valid = true;
    if (YAW && A.yaw_max > 0) {
      bool amb = false;  // (device trig, as mplx_rollout_device decides it; at rest no trig is evaluated)
      valid = P.heading_valid(nullptr, 0, cos(A.yaw_max), A.yaw.margin, A.yaw.tie_yaw, &amb);
    }
    valid = P.limits_valid(A, valid);
    const int cnt = W.count[k];
    if (P.wait_eligible(valid) && cnt >= 0 && (int64_t)cnt < W.S) {
      const int64_t e = k * W.S + cnt;
      W.action[e] = W.a0;
      W.cost[e] = P.wait_cost(A);  // env_map.h:164-165 with a traversal cost of 0
      if (W.hash) W.hash[e] = P.h_next;
      if (W.state) {
        double *o = W.state + e;
#pragma unroll
        for (int i = 0; i < D; i++) {
          o[(int64_t)(0 * D + i) * W.state_stride] = P.npos[i];
          o[(int64_t)(1 * D + i) * W.state_stride] = P.nvel[i];
          o[(int64_t)(2 * D + i) * W.state_stride] = P.nacc[i];
          o[(int64_t)(3 * D + i) * W.state_stride] = P.njrk[i];
        }
        o[(int64_t)(4 * D) * W.state_stride] = P.nyaw;
        o[(int64_t)(F - 1) * W.state_stride] = tp + A.dt;  // env_map.h:161
      }
      if (W.iters) W.iters[e] = 0;
      if (W.post.heur || W.post.flags) {
        MPLX_POST_GOAL(PG, W.post, D)
        double heur;
        unsigned int flags;
        dev::post_eval<D>(PG, P.h_next, P.npos, P.nvel, P.nacc, P.nyaw, &heur, &flags);
        if (W.post.heur) W.post.heur[e] = heur;
        if (W.post.flags) W.post.flags[e] = (uint8_t)flags;
      }
      W.count[k] = cnt + 1;
      added = true;
    }
  }
  const unsigned long long any = __ballot(added);
  if (W.n_added && any && (threadIdx.x & 63) == 0) atomicAdd(W.n_added, (unsigned long long)__popcll(any));
}

template <int D, int K, bool YAW>
hipError_t launch_one(const WaitArgs &a, hipStream_t s) {
  const int64_t blocks = (a.n_rows + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((lists_add_wait_kernel<D, K, YAW>), dim3((unsigned)blocks), dim3(kBlock), 0, s, a);
  return hipGetLastError();
}

template <int D>
hipError_t launch_dim(int control, const WaitArgs &a, hipStream_t s) {
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

hipError_t launch_lists_add_wait(int dim, int control, const WaitArgs &a, hipStream_t s) {
  if (a.n_rows <= 0) return hipSuccess;
  if (dim == 2) return launch_dim<2>(control, a, s);
  if (dim == 3) return launch_dim<3>(control, a, s);
  return hipErrorInvalidValue;
}

}  // namespace mplx
