// mplx_traj_device.h -- the segment look-up and one evaluated sample of a stored segment, shared by the kernels that read
// a segment table (traj_kernel.hip; limits_kernel.hip fills the waypoints of a loaded set with it; conflict_kernel.hip).
#ifndef MPLX_TRAJ_DEVICE_H
#define MPLX_TRAJ_DEVICE_H

#include "mplx_internal.h"
#include "mplx_pair_device.h"

namespace mplx {
namespace traj {

// One evaluated sample: the segment look-up and the polynomial values of trajectory.h:67-135.
template <int D>
struct Sample {
  double pos[D], vel[D], acc[D], jrk[D], yaw, yaw_dot;
};

// seg: the segment's rows for this trajectory (stride N); t: tau - taus[id], finite and >= 0.
// primitive.h:128-145 with c0 = 0 (its term is +0.0: the leading `0.0 +`), power by repeated multiply.
// POLY: a solved segment, rows c0 .. c5 per axis: all six terms of primitive.h:128-145, operation for operation.
// lambda, lambda_dot: Lambda::evaluate at the sample's virtual time (include/mplx_scale.h); 1 and 0 without a Lambda.
template <int D, bool COMMAND, bool WANT_ALL, bool POLY = false>
__device__ __forceinline__ void eval_segment(const double *seg, int64_t N, double t, Sample<D> &o, const double lambda = 1.0,
                                             const double lambda_dot = 0.0) {
  const double t3 = (t * t) * t, t4 = t3 * t;
  constexpr int NA = POLY ? 6 : 5;  // rows per axis
#pragma unroll
  for (int i = 0; i < D; i++) {
    const double *sa = seg + (int64_t)(NA * i + (POLY ? 1 : 0)) * N;
    const double c1 = sa[0 * N], c2 = sa[1 * N], c3 = sa[2 * N], c4 = sa[3 * N], c5 = sa[4 * N];
    double v, a, j;
    if (POLY) {
      const double c0 = seg[(int64_t)(NA * i) * N], t5 = t4 * t;
      o.pos[i] = ((((c0 / 120 * t5 + c1 / 24 * t4) + c2 / 6 * t3) + c3 / 2 * t * t) + c4 * t) + c5;
      v = (((c0 / 24 * t4 + c1 / 6 * t3) + c2 / 2 * t * t) + c3 * t) + c4;
      a = ((c0 / 6 * t3 + c1 / 2 * t * t) + c2 * t) + c3;
      j = (c0 / 2 * t * t + c1 * t) + c2;
    } else {
      o.pos[i] = ((((0.0 + c1 / 24 * t4) + c2 / 6 * t3) + c3 / 2 * t * t) + c4 * t) + c5;
      v = (((0.0 + c1 / 6 * t3) + c2 / 2 * t * t) + c3 * t) + c4;
      a = ((0.0 + c1 / 2 * t * t) + c2 * t) + c3;
      j = (0.0 + c1 * t) + c2;
    }
    if (!WANT_ALL) {
      o.vel[i] = v;  // (lambda = 1: v / 1)
      continue;
    }
    if (COMMAND) {
      // trajectory.h:119-124, operation for operation
      const double l3 = (1.0 * lambda) * lambda * lambda, l4 = l3 * lambda;
      o.vel[i] = v / lambda;
      o.acc[i] = a / lambda / lambda - o.vel[i] * lambda_dot / lambda / lambda / lambda;
      o.jrk[i] = j / lambda / lambda - 3 / l3 * o.acc[i] * o.acc[i] * lambda_dot + 3 / l4 * o.vel[i] * lambda_dot * lambda_dot;
    } else {
      o.vel[i] = v;
      o.acc[i] = a;
      o.jrk[i] = j;
    }
  }
  if (WANT_ALL) {
    const double uy = seg[(NA * D) * N], y0 = seg[(NA * D + 1) * N];
    o.yaw = dev::wrap_angle((0.0 + uy * t) + y0);
    o.yaw_dot = dev::wrap_angle(0.0 + uy);  // (yes: normalize_angle of the yaw rate, trajectory.h:126)
  }
}

// One segment of a chain: the primitive of (state s, control row up) per axis (primitive.h:34-50 through dev::Ax) and
// its rows c1 .. c5 per axis, then the yaw primitive's rate and yaw, stride N -- what eval_segment reads.  The chain
// launch (traj_kernel.hip) stores into the segment table with it; reserve_kernel.hip into registers (N = 1).
template <int D, int K>
__device__ __forceinline__ void chain_segment(const double *s, const double *up, double uy, double cyaw, dev::Ax<K> (&ax)[D],
                                              double *seg, int64_t N) {
#pragma unroll
  for (int i = 0; i < D; i++) ax[i].init(s[i], s[D + i], s[2 * D + i], s[3 * D + i], up[i]);
#pragma unroll
  for (int i = 0; i < D; i++) {
    seg[(5 * i + 0) * N] = ax[i].c1;
    seg[(5 * i + 1) * N] = ax[i].c2;
    seg[(5 * i + 2) * N] = ax[i].c3;
    seg[(5 * i + 3) * N] = ax[i].c4;
    seg[(5 * i + 4) * N] = ax[i].c5;
  }
  seg[(5 * D) * N] = uy;
  seg[(5 * D + 1) * N] = cyaw;
}

// COMMAND: the first id with tau >= taus[id] && tau <= taus[id+1]; WAYPOINT: ... && tau < taus[id+1], else the last.
// taus grow strictly (dt > 0), so the first match is the smallest id whose upper end admits tau.
// POLY (a solved set: every segment has its own duration): no guess, a bisection on the stored taus for the same id.
template <bool COMMAND, bool POLY = false>
__device__ __forceinline__ int find_segment(const double *taus, int64_t N, int S, double tau, double dt) {
  if (POLY) {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const double up = taus[(int64_t)(mid + 1) * N];
      if (COMMAND ? tau <= up : tau < up) hi = mid; else lo = mid + 1;
    }
    return lo;
  }
  double q = tau / dt;
  q = q >= 0.0 ? q : 0.0;  // (a NaN goes to 0)
  int g = q < (double)(S - 1) ? (int)q : S - 1;
  if (COMMAND) {
    while (g > 0 && tau <= taus[(int64_t)g * N]) g--;
    while (g < S - 1 && !(tau <= taus[(int64_t)(g + 1) * N])) g++;
  } else {
    while (g > 0 && tau < taus[(int64_t)g * N]) g--;
    while (g < S - 1 && !(tau < taus[(int64_t)(g + 1) * N])) g++;
  }
  return g;
}

}  // namespace traj
}  // namespace mplx
#endif
