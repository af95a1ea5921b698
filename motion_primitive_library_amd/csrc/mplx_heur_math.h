// mplx_heur_math.h -- the arithmetic of include/mplx_heur.h, written once for the device (heur_kernel.hip, the DYN
// instantiations of open_kernel.hip) and for a host build of the same expressions (MPLX_HD is empty without a HIP
// compiler): the dynamics-aware heuristic of PlannerBase::setHeurIgnoreDynamics(false).
//
// Reference: include/mpl_planner/common/env_base.h:56-211 (cal_heur).  heur::reference is its branches that need no
// Eigen solver -- ACC-ACC (:158-182), ACC-VEL (:184-206), VEL-VEL (:207-208) and the final else (:209-210) -- expression
// for expression on top of scale::quartic, under -ffp-contract=off.  It goes through cbrt / acos / cos, whose last bits
// are the C library's on the host and OCML's on the device, and `t < t_bar` turns such a bit into another candidate set:
// it is HOST ONLY, and nothing on the device calls it.
//
// heur::robust is this library's: the true minimum over t >= t_bar of the same cost functions, for VEL, ACC and JRK
// states, with + - * / sqrt fabs and comparisons only -- the same bits on the device, on the host and in the Python
// model (tests/heur_model.py), which is its specification.  Stated in include/mplx_heur.h.
//
// A state and a goal are 4D+1 doubles: pos[D] vel[D] acc[D] jrk[D] yaw (the rows of a Waypoint without its time).
#ifndef MPLX_HEUR_MATH_H
#define MPLX_HEUR_MATH_H

#include "mplx_scale_math.h"

#include <float.h>

namespace mplx {
namespace heur {

constexpr int kVel = 0x01, kAcc = 0x03, kJrk = 0x07;  // MPLX_VEL / _ACC / _JRK
constexpr int kBisect = 56;                            // MPLX_HEUR_BISECT

template <int D>
MPLX_HD double dot(const double *a, const double *b) {
  double s = a[0] * b[0];
#pragma unroll
  for (int i = 1; i < D; i++) s = s + a[i] * b[i];
  return s;
}

template <int D>
MPLX_HD double linf(const double *s, const double *g) {
  double m = 0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    const double d = fabs(s[i] - g[i]);
    m = d > m ? d : m;
  }
  return m;
}

// ---- REFERENCE (host only) ------------------------------------------------------------------------------------------

// env_base.h:169-181 / :194-206: the candidates of quartic in its order, then t_bar
MPLX_HD double reference_quartic_min(double c1, double c2, double c3, double w, double t_bar) {
  const scale::Roots4 ts = scale::quartic(w, 0.0, c3, c2, c1);
  double cost = DBL_MAX;
#pragma unroll
  for (int i = 0; i < 5; i++) {
    if (i < 4 && !((ts.mask >> i) & 1u)) continue;
    const double t = i < 4 ? ts.r[i] : t_bar;
    if (t < t_bar) continue;
    const double c = -c1 / 3 / t / t / t - c2 / 2 / t / t - c3 / t + w * t;
    if (c < cost) cost = c;
  }
  return cost;
}

// cal_heur with heur_ignore_dynamics_ == false, control flags compared exactly (ACCxYAW is no ACC: the else branch).  A
// JRK state with a JRK, ACC or VEL goal goes through Eigen's PolynomialSolver in the reference: *unsupported is set and
// the value is NaN -- the callers refuse such a configuration before they get here.
template <int D>
MPLX_HD double reference(const double *s, const double *g, int control, int goal_control, double w, double v_max, bool *unsupported) {
  *unsupported = false;
  double dp[D], vs[D];
#pragma unroll
  for (int i = 0; i < D; i++) dp[i] = g[i] - s[i];
  const double *v0 = s + D, *v1 = g + D;
  if (control == kJrk && (goal_control == kJrk || goal_control == kAcc || goal_control == kVel)) {
    *unsupported = true;
    return NAN;
  }
  if (control == kAcc && goal_control == kAcc) {
#pragma unroll
    for (int i = 0; i < D; i++) vs[i] = v0[i] + v1[i];
    const double c1 = -36 * dot<D>(dp, dp);
    const double c2 = 24 * dot<D>(vs, dp);
    const double c3 = -4 * (dot<D>(v0, v0) + dot<D>(v0, v1) + dot<D>(v1, v1));
    return reference_quartic_min(c1, c2, c3, w, linf<D>(s, g) / v_max);
  }
  if (control == kAcc && goal_control == kVel) {
    const double c1 = -9 * dot<D>(dp, dp);
    const double c2 = 12 * dot<D>(v0, dp);
    const double c3 = -3 * dot<D>(v0, v0);
    return reference_quartic_min(c1, c2, c3, w, linf<D>(s, g) / v_max);
  }
  double sp[D];
#pragma unroll
  for (int i = 0; i < D; i++) sp[i] = s[i] - g[i];
  const double norm = sqrt(dot<D>(sp, sp));
  if (control == kVel && goal_control == kVel) return (w + 1) * norm;
  return w * norm / v_max;
}

// ---- ROBUST ---------------------------------------------------------------------------------------------------------

// Horner, one multiply and one add per coefficient
template <int M>
MPLX_HD double horner(const double (&q)[M + 1], double t) {
  double r = q[M];
#pragma unroll
  for (int k = M - 1; k >= 0; k--) r = r * t + q[k];
  return r;
}

constexpr int falling(int n, int k) { return k == 0 ? 1 : n * falling(n - 1, k - 1); }  // n (n - 1) .. (n - k + 1)

// Derivative-chain isolation of the real roots of p (degree N, p[N] > 0) in (lo, hi]: Chain<N, M> leaves in x[0 .. M) the
// break points that the roots of the (N - M)-th derivative, of degree M, give -- in ascending order, every one in
// [lo, hi].  Between two neighbours of lo, x'[0 .. M - 1), hi (the break points of the derivative above) the polynomial
// is monotone, so a sign change is exactly one root and kBisect halvings find it; an interval without one hands its
// upper end on, which splits a monotone stretch of the next level in two and loses nothing.  ok[i]: x[i] is a root.
// Every loop has a compile-time trip count, every index is a constant after unrolling, and every lane does the same work
// whatever its number of roots: the intervals of a level are advanced together, one halving at a time.
template <int N, int M>
struct Chain {
  static MPLX_HD void run(const double (&p)[N + 1], double lo, double hi, double (&x)[M], bool (&ok)[M]) {
    double xd[M - 1];
    bool okd[M - 1];
    Chain<N, M - 1>::run(p, lo, hi, xd, okd);
    double q[M + 1];
#pragma unroll
    for (int j = 0; j <= M; j++) q[j] = p[j + (N - M)] * (double)falling(j + (N - M), N - M);
    double a[M], b[M];
    bool na[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
      a[i] = i == 0 ? lo : xd[i - 1];
      b[i] = i == M - 1 ? hi : xd[i];
      na[i] = horner<M>(q, a[i]) < 0;
      ok[i] = na[i] != (horner<M>(q, b[i]) < 0);
      x[i] = b[i];
    }
    for (int it = 0; it < kBisect; it++) {
#pragma unroll
      for (int i = 0; i < M; i++) {
        const double m = a[i] + (b[i] - a[i]) * 0.5;
        const bool same = (horner<M>(q, m) < 0) == na[i];
        a[i] = same ? m : a[i];
        b[i] = same ? b[i] : m;
      }
    }
#pragma unroll
    for (int i = 0; i < M; i++) x[i] = ok[i] ? b[i] : x[i];
  }
};
template <int N>
struct Chain<N, 1> {  // the linear derivative: its root, clamped into [lo, hi]
  static MPLX_HD void run(const double (&p)[N + 1], double lo, double hi, double (&x)[1], bool (&ok)[1]) {
    const double q0 = p[N - 1] * (double)falling(N - 1, N - 1), q1 = p[N] * (double)falling(N, N - 1);
    double r = -q0 / q1;
    r = r > lo ? r : lo;  // (a NaN goes to lo)
    r = r < hi ? r : hi;
    x[0] = r;
    ok[0] = true;
  }
};

// Cauchy's bound: every root of p lies in |t| <= 1 + max |p[k] / p[N]|
template <int N>
MPLX_HD double cauchy(const double (&p)[N + 1]) {
  double m = 0;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const double r = fabs(p[k] / p[N]);
    m = r > m ? r : m;
  }
  return 1.0 + m;
}

// min over {t_bar if > 0} and the roots of p in (t_bar, T_hi] of C; +inf when there is no candidate.  COST(t) is C.
template <int N, class COST>
MPLX_HD double min_cost(const double (&p)[N + 1], double t_bar, const COST &cost) {
  double x[N];
  bool ok[N];
  const double hi = cauchy<N>(p);
  Chain<N, N>::run(p, t_bar, hi > t_bar ? hi : t_bar, x, ok);
  double best = INFINITY;
  if (t_bar > 0) best = cost(t_bar);
#pragma unroll
  for (int i = 0; i < N; i++) {
    const double c = cost(x[i]);  // (x[i] >= t_bar, and > 0 where ok: a sign change lies above lo)
    if (ok[i] && x[i] > 0 && c < best) best = c;
  }
  return best;
}

struct CostAcc {  // env_base.h:177, :202
  double c1, c2, c3, w;
  MPLX_HD double operator()(double t) const { return -c1 / 3 / t / t / t - c2 / 2 / t / t - c3 / t + w * t; }
};
struct CostJrk {  // env_base.h:91-92
  double a, c, d, e, f, g;
  MPLX_HD double operator()(double t) const {
    return a * t - c / t - d / 2 / t / t - e / 3 / t / t / t - f / 4 / t / t / t / t - g / 5 / t / t / t / t / t;
  }
};

// The base control of a flag: without its yaw bit.
MPLX_HD int base_control(int control) { return control & 0x0f; }

// h of one state that is not the goal's own lattice state (the caller keeps that one at 0).  w > 0.
template <int D>
MPLX_HD double robust(const double *s, const double *g, int control, int goal_control, double w, double v_max) {
  double fin = 0;  // 0 for finite input, NaN otherwise
#pragma unroll
  for (int i = 0; i < 3 * D; i++) fin = fin + ((s[i] - s[i]) + (g[i] - g[i]));
  fin = fin + ((w - w) + (v_max - v_max));
  const double L = linf<D>(s, g);
  const double h0 = v_max > 0 ? w * L / v_max : w * L;  // the default: dev::post_eval's expression
  if (!(fin == 0)) return NAN;
  const double t_bar = v_max > 0 ? L / v_max : 0.0;
  const int cs = base_control(control), cg = base_control(goal_control ? goal_control : control);
  double dp[D];
#pragma unroll
  for (int i = 0; i < D; i++) dp[i] = g[i] - s[i];
  const double *v0 = s + D, *v1 = g + D, *a0 = s + 2 * D, *a1 = g + 2 * D;
  double best;
  if (cs == kVel && cg == kVel) {
    const double pp = dot<D>(dp, dp);
    const double ts = sqrt(pp) / sqrt(w);
    best = INFINITY;
    if (t_bar > 0) best = pp / t_bar + w * t_bar;
    if (ts > t_bar) {
      const double c = pp / ts + w * ts;
      best = c < best ? c : best;
    }
  } else if (cs == kAcc && (cg == kAcc || cg == kVel)) {
    CostAcc C;
    C.w = w;
    if (cg == kAcc) {
      double vs[D];
#pragma unroll
      for (int i = 0; i < D; i++) vs[i] = v0[i] + v1[i];
      C.c1 = -36 * dot<D>(dp, dp);
      C.c2 = 24 * dot<D>(vs, dp);
      C.c3 = -4 * (dot<D>(v0, v0) + dot<D>(v0, v1) + dot<D>(v1, v1));
    } else {
      C.c1 = -9 * dot<D>(dp, dp);
      C.c2 = 12 * dot<D>(v0, dp);
      C.c3 = -3 * dot<D>(v0, v0);
    }
    const double p[5] = {C.c1, C.c2, C.c3, 0.0, w};
    best = min_cost<4>(p, t_bar, C);
  } else if (cs == kJrk && (cg == kJrk || cg == kAcc || cg == kVel)) {
    CostJrk C;
    C.a = w;
    if (cg == kJrk) {  // env_base.h:75-81
      double da[D], vs[D];
#pragma unroll
      for (int i = 0; i < D; i++) {
        da[i] = a0[i] - a1[i];
        vs[i] = v0[i] + v1[i];
      }
      C.c = -9 * dot<D>(a0, a0) + 6 * dot<D>(a0, a1) - 9 * dot<D>(a1, a1);
      C.d = -144 * dot<D>(a0, v0) - 96 * dot<D>(a0, v1) + 96 * dot<D>(a1, v0) + 144 * dot<D>(a1, v1);
      C.e = 360 * dot<D>(da, dp) - 576 * dot<D>(v0, v0) - 1008 * dot<D>(v0, v1) - 576 * dot<D>(v1, v1);
      C.f = 2880 * dot<D>(dp, vs);
      C.g = -3600 * dot<D>(dp, dp);
    } else if (cg == kAcc) {  // env_base.h:106-111
      double vm[D];
#pragma unroll
      for (int i = 0; i < D; i++) vm[i] = 1600 * v0[i] + 960 * v1[i];
      C.c = -8 * dot<D>(a0, a0);
      C.d = -112 * dot<D>(a0, v0) - 48 * dot<D>(a0, v1);
      C.e = 240 * dot<D>(a0, dp) - 384 * dot<D>(v0, v0) - 432 * dot<D>(v0, v1) - 144 * dot<D>(v1, v1);
      C.f = dot<D>(dp, vm);
      C.g = -1600 * dot<D>(dp, dp);
    } else {  // env_base.h:136-140
      C.c = -5 * dot<D>(a0, a0);
      C.d = -40 * dot<D>(a0, v0);
      C.e = 60 * dot<D>(a0, dp) - 60 * dot<D>(v0, v0);
      C.f = 160 * dot<D>(dp, v0);
      C.g = -100 * dot<D>(dp, dp);
    }
    const double p[7] = {C.g, C.f, C.e, C.d, C.c, 0.0, w};
    best = min_cost<6>(p, t_bar, C);
  } else {
    return h0;
  }
  return (best < INFINITY && best > h0) ? best : h0;  // max(default, min C); no candidate: the default
}

}  // namespace heur
}  // namespace mplx
#endif
