// mplx_pair_device.h -- the arithmetic of ONE (state, control input) pair of MPL::env_map<Dim>::get_succ
//   reference include/mpl_planner/env/env_map.h:147-172 (get_succ)
//   reference include/mpl_planner/env/env_map.h:90-132  (traverse_primitive)
// as __device__ functions for kernels that evaluate whole pairs one lane each: rollout_kernel.hip (one pair per step
// of an action sequence), wait_kernel.hip, replan_kernel.hip are built on Pair; the helpers below and dev::Ax are the
// dense kernel's too.  The rules of that arithmetic are stated here, against the specification in SURVEY.md
// Appendix A.  The result must be bit-identical to the CPU path, so:
//   * every unit that includes this file is compiled with -ffp-contract=off (no FMA contraction) and without any
//     fast-math flag; every product / sum below is one IEEE binary64 operation in the reference's evaluation order;
//   * divisions are true divisions (never multiplication by a reciprocal);
//   * the sample time is accumulated (t += dt), never computed as k*dt (env_map.h:97-99 runs n or n+1 iterations
//     depending on rounding);
//   * structurally-zero coefficient terms are dropped only where that cannot change a bit of the result (SURVEY.md
//     Appendix A-7); the emitted successor state keeps the leading `0.0 +` so that signed zeros match.
// The per-axis polynomial is dev::Ax<K> (mplx_device_common.h), with its derivations.
//
// expand_kernel.hip's kernel body still spells Pair's four steps out by hand, for a measured reason (MI355X, C4:
// 65 536 nodes x 729 ACC controls, medians, ms; profiles/pair_arithmetic_refactor.txt).  The dense kernel alone:
// 3.264 and 3.265 in two runs of the body as it is, 3.362 with the body built on Pair (+3.0 %); C4 through the DENSE
// lists route 5.123 and 5.122 against 5.255 (+2.6 %), the 17^3 table 5.270 and 5.295 against 5.361.  Registers,
// scratch and occupancy are the same in all 16 instantiations; with Pair the optimiser evaluates the sample's
// velocity in the traversal loop whether or not a cost term reads it.  The body on dev::Ax and the helpers of this
// file, without the struct, measures 3.248 beside 3.247 -- that is what the dense kernel uses, and
// tests/test_gpu_rollout.py compares the two kernels directly (dense slot (node, a) == rollout of one step).
#ifndef MPLX_PAIR_DEVICE_H
#define MPLX_PAIR_DEVICE_H

#include "mplx_internal.h"
#include "mplx_device_common.h"  // Ax, fold, wrap_angle; near_limit / heading_unit of the yaw paths

#include <math.h>

namespace mplx {
namespace pair {

// ---------------------------------------------------------------- lattice hash
// `int id = std::round(x / q)`: round half away from zero, then value-convert.
// (a true division, and the yaw: not dev::quantise's refined reciprocal on purpose)
__device__ __forceinline__ int quantise(double x, double q) { return (int)round(x / q); }

template <int D, int K, bool YAW>
__device__ __forceinline__ uint64_t lattice_hash(const double *pos, const double *vel,
                                                 const double *acc, const double *jrk, double yaw) {
  uint64_t h = 0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    dev::fold(h, quantise(pos[i], 0.01));
    if (K >= 2) dev::fold(h, quantise(vel[i], 0.1));
    if (K >= 3) dev::fold(h, quantise(acc[i], 0.1));
    if (K >= 4) dev::fold(h, quantise(jrk[i], 0.1));
  }
  if (YAW) dev::fold(h, quantise(yaw, 0.1));
  return h;
}

// primitive.h:504-525, one end of the primitive.  cs: the host libm's {cos(yaw), sin(yaw)} in the override pass of
// the yaw pinning (YawPin, mplx_internal.h), else null; *amb: the decision is within `margin` of the threshold.
__device__ __forceinline__ bool heading_ok(double vx, double vy, double yaw, double cos_lim, const double *cs,
                                           double margin, double tie_yaw, bool *amb) {
  if (vx != 0 || vy != 0) {
    const double s = sqrt(vx * vx + vy * vy);
    const double c = cs ? cs[0] : cos(yaw), sn = cs ? cs[1] : sin(yaw);
    const double d = vx / s * c + vy / s * sn;
    *amb = *amb || mplx::dev::near_limit(d, cos_lim, margin, vy, yaw, tie_yaw);
    if (d < cos_lim) return false;
  }
  return true;
}

// ------------------------------------------------------------------ one pair
// The caller fills the current state (cpos .. cyaw; rows its control order does not read are 0.0) and calls, in this
// order: init() -- the primitive, the successor state tn = pr.evaluate(dt), both lattice hashes, max_vel per axis --,
// heading_valid() where a heading limit applies, limits_valid(), classify().
template <int D, int K, bool YAW>
struct Pair {
  double cpos[D], cvel[D], cacc[D], cjrk[D], cyaw;
  double npos[D], nvel[D], nacc[D], njrk[D], nyaw;
  double uyaw;
  dev::Ax<K> ax[D];
  uint64_t h_next, h_curr;
  double mv[D], max_v;

  // u: the control's D spatial entries; uy: its yaw rate (YAW only)
  __device__ __forceinline__ void init(const double *u, double uy, double T) {
#pragma unroll
    for (int i = 0; i < D; i++) ax[i].init(cpos[i], cvel[i], cacc[i], cjrk[i], u[i]);
    uyaw = YAW ? uy : 0.0;

    // ---- successor state tn = pr.evaluate(dt)  (env_map.h:157, primitive.h:321-331)
#pragma unroll
    for (int i = 0; i < D; i++) {
      npos[i] = ax[i].template pos<true>(T);
      nvel[i] = ax[i].template vel<true>(T);
      nacc[i] = ax[i].template acc<true>(T);
      njrk[i] = ax[i].template jrk<true>(T);
    }
    nyaw = 0.0;
    if (YAW) nyaw = dev::wrap_angle((0.0 + uyaw * T) + cyaw);

    h_next = lattice_hash<D, K, YAW>(npos, nvel, nacc, njrk, nyaw);
    h_curr = lattice_hash<D, K, YAW>(cpos, cvel, cacc, cjrk, cyaw);

    // ---- dynamic limits (primitive.h:450-475); max_vel is needed again by the
    //      traversal, so it is computed once here
    max_v = 0;
#pragma unroll
    for (int i = 0; i < D; i++) {
      mv[i] = ax[i].max_vel(T);
      if (mv[i] > max_v) max_v = mv[i];
    }
  }

  // validate_yaw at both ends of the primitive (primitive.h:504-525); call only when YAW && yaw_max > 0.
  // tab: override pass of the yaw pinning -- {cos, sin} of yaw(0), then of yaw(T) for every control (ci), all from the
  // host libm --, else null; cos_lim: cos(yaw_max) from the same library as the table.
  __device__ __forceinline__ bool heading_valid(const double *tab, int ci, double cos_lim, double margin, double tie_yaw,
                                                bool *amb) const {
    // evaluate(0): vel = 0.0 + c4 terms, yaw = wrap(0.0 + uyaw*0 + yaw)
    const double y0 = dev::wrap_angle((0.0 + uyaw * 0.0) + cyaw);
    const bool ok0 = heading_ok(ax[0].template vel<true>(0.0), ax[1].template vel<true>(0.0), y0, cos_lim,
                                tab ? tab : nullptr, margin, tie_yaw, amb);
    const bool okT = heading_ok(nvel[0], nvel[1], nyaw, cos_lim, tab ? tab + 2 + 2 * ci : nullptr, margin,
                                tie_yaw, amb);
    return ok0 && okT;
  }

  __device__ __forceinline__ bool limits_valid(const ExpandArgs &A, bool valid) const {
    const double T = A.dt;
    if (K >= 2 && A.v_max > 0) {
#pragma unroll
      for (int i = 0; i < D; i++) valid = valid && !(mv[i] > A.v_max);
    }
    if (K >= 3 && A.a_max > 0) {
#pragma unroll
      for (int i = 0; i < D; i++) valid = valid && !(ax[i].max_acc(T) > A.a_max);
    }
    if (K >= 4 && A.j_max > 0) {
#pragma unroll
      for (int i = 0; i < D; i++) valid = valid && !(ax[i].max_jrk(T) > A.j_max);
    }
    return valid;
  }

  // Slot status, cost (+inf unless FINITE) and sample-loop iteration count of the pair.
  __device__ __forceinline__ void classify(const ExpandArgs &A, bool valid, uint8_t *st_out, double *cost_out,
                                           int *iters_out) const {
    const double T = A.dt;
    uint8_t st;
    double cost = INFINITY;
    int iters = 0;
    if (h_next == h_curr) {
      st = 0;  // MPLX_SLOT_SKIP_SAME
    } else if (!valid) {
      st = 3;  // MPLX_SLOT_SKIP_DYN
    } else {
      // ---- traverse_primitive (env_map.h:90-132), skipped when the position
      //      does not change at all (env_map.h:163)
      bool same_pos = true;
#pragma unroll
      for (int i = 0; i < D; i++) same_pos = same_pos && (cpos[i] == npos[i]);
      double c = 0;
      bool blocked = false;
      if (!same_pos) {
        int n = (int)ceil(max_v * T / A.res);
        n = n < 5 ? 5 : n;
        const double sdt = T / n;
        const double org[3] = {A.org0, A.org1, A.org2};
        const int dims[3] = {A.dim0, A.dim1, A.dim2};
        const bool want_vel = (A.pot != nullptr && A.grad_w != 0) || (YAW && A.wyaw > 0);
        for (double t = 0; t < T; t += sdt) {
          iters++;
          int cell[D];
          bool outside = false;
#pragma unroll
          for (int i = 0; i < D; i++) {
            // map_util.h:103-108
            cell[i] = (int)round((ax[i].template pos<false>(t) - org[i]) / A.res - 0.5);
            outside = outside || cell[i] < 0 || cell[i] >= dims[i];
          }
          if (outside) { blocked = true; break; }
          int64_t idx = cell[0] + (int64_t)dims[0] * cell[1];
          if (D == 3) idx += (int64_t)dims[0] * dims[1] * cell[2];
          if (A.region != nullptr && !((A.region[idx >> 5] >> (idx & 31)) & 1u)) { blocked = true; break; }
          double vs[D];
          if (want_vel) {
#pragma unroll
            for (int i = 0; i < D; i++) vs[i] = ax[i].template vel<false>(t);
          }
          if (A.pot != nullptr) {
            const int pv = A.pot[idx];
            if (pv < 100 && pv > 0) {
              double gterm = 0;
              if (A.grad_w != 0) {
                double q = 0;
#pragma unroll
                for (int i = 0; i < D; i++) q += vs[i] * vs[i];
                gterm = A.grad_w * sqrt(q);
                c += sdt * (A.pot_w * pv + gterm);
              } else {
                // gradient_weight * norm is an exact +0 when the weight is 0
                c += sdt * (A.pot_w * pv + 0.0);
              }
            } else if (pv >= 100) { blocked = true; break; }
          } else if (A.map[idx] == 100) { blocked = true; break; }
          if (YAW && A.wyaw > 0) {
            double ux, uy;
            if (mplx::dev::heading_unit(vs[0], vs[1], ux, uy)) {  // (mplx_device_common.h: the same unit vector in every kernel)
              const double yw = dev::wrap_angle(uyaw * t + cyaw);
              const double v_value = 1 - (ux * cos(yw) + uy * sin(yw));
              c += A.wyaw * v_value * sdt;
            }
          }
        }
      }
      if (blocked) {
        st = 2;  // MPLX_SLOT_BLOCKED
      } else {
        // env_map.h:164-165, env_base.h:343-345: cost += J + w*dt
        double J = 0;
#pragma unroll
        for (int i = 0; i < D; i++) J += ax[i].effort(T);
        cost = c + (J + A.w * A.dt);
        st = 1;  // MPLX_SLOT_FINITE
      }
    }
    *st_out = st;
    *cost_out = cost;
    *iters_out = iters;
  }

  // Wait edges (include/mplx_wait.h), for the zero control: the pair is the successor get_succ drops, it is valid
  // (heading and limits) and the position does not move at all.  wait_kernel.hip appends the entry by these two; the
  // timed rebase (replan_kernel.hip) tests a kept wait edge by them.
  __device__ __forceinline__ bool wait_eligible(bool valid) const {
    bool same_pos = true;
#pragma unroll
    for (int i = 0; i < D; i++) same_pos = same_pos && (cpos[i] == npos[i]);
    return h_next == h_curr && valid && same_pos;
  }
  // env_map.h:164-165 with a traversal cost of 0 (classify's expression)
  __device__ __forceinline__ double wait_cost(const ExpandArgs &A) const {
    double J = 0;
#pragma unroll
    for (int i = 0; i < D; i++) J += ax[i].effort(A.dt);
    const double c = 0;
    return c + (J + A.w * A.dt);
  }
};

}  // namespace pair
}  // namespace mplx
#endif
