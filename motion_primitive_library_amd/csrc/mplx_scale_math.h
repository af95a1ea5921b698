// mplx_scale_math.h -- the arithmetic of include/mplx_scale.h, written once for the device (scale_kernel.hip, the Lambda
// instantiations of traj_kernel.hip) and for a host build of the same expressions (MPLX_HD is empty without a HIP
// compiler): quartic and the five-argument solve next to cubic, LambdaSeg, Lambda::getT / getTau / evaluate, and the
// candidates of scale_down.
//
// Reference: include/mpl_basis/math.h:69-110 (quartic), 117-131 (solve), include/mpl_basis/lambda.h:29-67 (LambdaSeg),
// 116-161 (Lambda::evaluate, getT, getTau).  Expression for expression, under -ffp-contract=off, power() as repeated
// multiplication.  The ROBUST forms and the Hermite coefficients are this library's, stated in include/mplx_scale.h.
//
// A Lambda is read through a loader ld(s, f): field f of segment s -- 0 .. 3: a3 a2 a1 a0, 4: ti, 5: tf, 6: getT(ti) of
// the segment's own quartic, 7: dT -- so the device reads its problem-minor table and the host an array.
#ifndef MPLX_SCALE_MATH_H
#define MPLX_SCALE_MATH_H

#include "mplx_limits_math.h"

#include <stdint.h>

namespace mplx {
namespace scale {

#if defined(__HIPCC__)
// field f of segment s of one problem of a problem-minor Lambda table: seg points at the problem's column, n is the stride
struct TableLoader {
  const double *seg;
  int64_t n;
  __device__ __forceinline__ double operator()(int s, int f) const { return seg[(int64_t)(s * 8 + f) * n]; }
};
#endif

constexpr int kMaxSegs = 8;   // MPLX_LAMBDA_MAX_SEGS
constexpr int kNewton = 3;    // MPLX_LAMBDA_NEWTON
constexpr int kBadPoints = 32, kNotPositive = 64;  // MPLX_LAMBDA_BAD_POINTS / _NOT_POSITIVE

// up to four roots in the order the reference returns them; bit i of mask: r[i] was returned
struct Roots4 {
  double r[4];
  unsigned mask;
};

// math.h:69-110: a t^4 + b t^3 + c t^2 + d t + e = 0.  The resolvent cubic always returns a root; its first one is
// taken.  A NaN r is not < 0: R, D and E are then NaN and nothing is returned, as in the reference.
MPLX_HD Roots4 quartic(double a, double b, double c, double d, double e) {
  Roots4 o{{0.0, 0.0, 0.0, 0.0}, 0};
  const double a3 = b / a, a2 = c / a, a1 = d / a, a0 = e / a;
  const limits::Roots ys = limits::cubic<false>(1.0, -a2, a1 * a3 - 4 * a0, 4 * a2 * a0 - a1 * a1 - a3 * a3 * a0);
  const double y1 = ys.r[0];
  const double r = a3 * a3 / 4 - a2 + y1;
  if (r < 0) return o;
  const double R = sqrt(r);
  double D, E;
  if (R != 0) {
    D = sqrt(0.75 * a3 * a3 - R * R - 2 * a2 + 0.25 * (4 * a3 * a2 - 8 * a1 - a3 * a3 * a3) / R);
    E = sqrt(0.75 * a3 * a3 - R * R - 2 * a2 - 0.25 * (4 * a3 * a2 - 8 * a1 - a3 * a3 * a3) / R);
  } else {
    D = sqrt(0.75 * a3 * a3 - 2 * a2 + 2 * sqrt(y1 * y1 - 4 * a0));
    E = sqrt(0.75 * a3 * a3 - 2 * a2 - 2 * sqrt(y1 * y1 - 4 * a0));
  }
  if (!(D != D)) {
    o.r[0] = -a3 / 4 + R / 2 + D / 2;
    o.r[1] = -a3 / 4 + R / 2 - D / 2;
    o.mask |= 3u;
  }
  if (!(E != E)) {
    o.r[2] = -a3 / 4 - R / 2 + E / 2;
    o.r[3] = -a3 / 4 - R / 2 - E / 2;
    o.mask |= 12u;
  }
  return o;
}

// math.h:117-131, all five arguments
MPLX_HD Roots4 solve5(double a, double b, double c, double d, double e) {
  if (a != 0) return quartic(a, b, c, d, e);
  const limits::Roots t = limits::solve<false>(b, c, d, e);
  Roots4 o{{t.r[0], t.r[1], t.r[2], 0.0}, (1u << t.n) - 1u};
  return o;
}

// lambda.h:57-60 and 52-53 for one segment, a = a3 a2 a1 a0
MPLX_HD double seg_getT(const double (&a)[4], double t) {
  const double t3 = (t * t) * t, t4 = t3 * t;
  return ((a[0] / 4 * t4 + a[1] / 3 * t3) + a[2] / 2 * t * t) + a[3] * t;
}
MPLX_HD double seg_lambda(const double (&a)[4], double tau) {
  const double t3 = (tau * tau) * tau;
  return ((a[0] * t3 + a[1] * tau * tau) + a[2] * tau) + a[3];
}
MPLX_HD double seg_lambda_dot(const double (&a)[4], double tau) { return (3 * a[0] * tau * tau + 2 * a[1] * tau) + a[2]; }

MPLX_HD bool finite3(double x, double y, double z) {
  const double s = (x - x) + (y - y) + (z - z);  // 0 for finite values, NaN otherwise
  return s == 0;
}

// One LambdaSeg from two virtual points: the Hermite cubic of include/mplx_scale.h, the 1e-5 clamp (REFERENCE), ti, tf,
// getT(ti), dT (lambda.h:38-46), and the checks of the mode.  Returns the status bits; o is complete either way.
MPLX_HD int build_seg(double p1, double v1, double t1, double p2, double v2, double t2, bool robust, double (&o)[8]) {
  const double h = t2 - t1, m = (p2 - p1) / h;
  const double c3 = ((v1 + v2) - 2 * m) / (h * h), c2 = ((3 * m - 2 * v1) - v2) / h;
  double a[4];
  a[0] = c3;
  a[1] = c2 - 3 * c3 * t1;
  a[2] = (v1 - 2 * c2 * t1) + 3 * c3 * t1 * t1;
  a[3] = ((p1 - v1 * t1) + c2 * t1 * t1) - c3 * t1 * t1 * t1;
  if (!robust) {
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (fabs(a[i]) < 1e-5) a[i] = 0;
  }
  const double g0 = seg_getT(a, t1);
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
  o[4] = t1; o[5] = t2; o[6] = g0;
  o[7] = seg_getT(a, t2) - g0;
  if (!finite3(p1, v1, t1) || !finite3(p2, v2, t2)) return kBadPoints;
  if (!robust) return 0;
  if (!(t2 > t1) || !(p1 > 0) || !(p2 > 0)) return kBadPoints;
  // the minimum of the cubic over [t1, t2]: the ends and the roots of its derivative inside
  bool pos = seg_lambda(a, t1) > 0 && seg_lambda(a, t2) > 0;
  limits::Roots ts{{0.0, 0.0, 0.0}, 0};
  if (3 * a[0] != 0) {
    ts = limits::quad(3 * a[0], 2 * a[1], a[2]);
  } else if (2 * a[1] != 0) {
    ts.r[0] = -a[2] / (2 * a[1]);
    ts.n = 1;
  }
#pragma unroll
  for (int i = 0; i < 2; i++) {
    if (i >= ts.n) continue;
    const double r = ts.r[i];
    if (r > t1 && r < t2 && !(seg_lambda(a, r) > 0)) pos = false;
  }
  return pos ? 0 : kNotPositive;
}

template <class L>
MPLX_HD void load_a(const L &ld, int s, double (&a)[4]) {
  a[0] = ld(s, 0); a[1] = ld(s, 1); a[2] = ld(s, 2); a[3] = ld(s, 3);
}

// Lambda::getT, lambda.h:127-138
template <class L>
MPLX_HD double lambda_getT(const L &ld, int n, double tau) {
  double T = 0;
  for (int s = 0; s < n; s++) {
    if (tau >= ld(s, 4) && tau <= ld(s, 5)) {
      double a[4];
      load_a(ld, s, a);
      return T + (seg_getT(a, tau) - ld(s, 6));
    }
    T = T + ld(s, 7);
  }
  return T;
}

// Lambda::evaluate, lambda.h:116-125.  No segment: zeros (REFERENCE), the last segment (ROBUST).
template <class L>
MPLX_HD void lambda_eval(const L &ld, int n, double tau, bool robust, double *lam, double *lam_dot) {
  int s = -1;
  for (int i = 0; i < n && s < 0; i++)
    if (tau >= ld(i, 4) && tau < ld(i, 5)) s = i;
  if (s < 0) {
    if (!robust) {
      *lam = 0.0;
      *lam_dot = 0.0;
      return;
    }
    s = n - 1;
  }
  double a[4];
  load_a(ld, s, a);
  *lam = seg_lambda(a, tau);
  *lam_dot = seg_lambda_dot(a, tau);
}

// Lambda::getTau, lambda.h:140-161: -1 and found = false where no segment gives a root inside itself
template <class L>
MPLX_HD double get_tau_reference(const L &ld, int n, double t, bool *found) {
  double T = 0;
  for (int s = 0; s < n; s++) {
    const double dT = ld(s, 7);
    if (t >= T && t <= T + dT) {
      const double ti = ld(s, 4), tf = ld(s, 5);
      const Roots4 ts = solve5(ld(s, 0) / 4, ld(s, 1) / 3, ld(s, 2) / 2, ld(s, 3), T - t - ld(s, 6));
      double hit = 0.0;
      bool have = false;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const double it = ts.r[i];
        if (!have && ((ts.mask >> i) & 1u) && it >= ti && it <= tf) {
          have = true;
          hit = it;
        }
      }
      if (have) {
        *found = true;
        return hit;
      }
    }
    T = T + dT;
  }
  *found = false;
  return -1.0;
}

// The ROBUST inverse of include/mplx_scale.h.  t is finite; total = Ts[S]; tau_end = taus[S].
template <class L>
MPLX_HD double get_tau_robust(const L &ld, int n, double t, double total, double tau_end) {
  if (!(t > 0)) return 0.0;
  if (t >= total) return tau_end;
  double T0 = 0;
  int s = 0;
  for (; s < n - 1; s++) {
    const double dT = ld(s, 7);
    if (t <= T0 + dT) break;
    T0 = T0 + dT;
  }
  double a[4];
  load_a(ld, s, a);
  const double ti = ld(s, 4), tf = ld(s, 5), g0 = ld(s, 6), dT = ld(s, 7);
  const Roots4 ts = solve5(a[0] / 4, a[1] / 3, a[2] / 2, a[3], T0 - t - g0);
  double best = ti + (t - T0) / dT * (tf - ti), dist = INFINITY;  // the linear guess
#pragma unroll
  for (int i = 0; i < 4; i++) {
    if (!((ts.mask >> i) & 1u)) continue;
    const double r = ts.r[i];
    const double d = r < ti ? ti - r : (r > tf ? r - tf : (r == r ? 0.0 : (double)INFINITY));
    if (d < dist) {
      dist = d;
      best = r;
    }
  }
  double tau = best >= ti ? best : ti;  // (a NaN goes to ti)
  tau = tau > tf ? tf : tau;
  for (int it = 0; it < kNewton; it++) {
    const double step = ((seg_getT(a, tau) - g0) + T0 - t) / seg_lambda(a, tau);
    if (fabs(step) < INFINITY) tau = tau - step;  // (not for a NaN or an infinite step)
    tau = tau >= ti ? tau : ti;
    tau = tau > tf ? tf : tau;
  }
  return tau;
}

// Uniform sample i of N: i * (total / N) (trajectory.h:233-234).  Under a ROBUST Lambda sample N is the total itself: N *
// (total / N) can fall an ulp short of it, and the last sample is the END state.
MPLX_HD double uniform_time(int64_t i, int n_uniform, double step, double total, bool robust_lambda) {
  return (robust_lambda && i == (int64_t)n_uniform) ? total : (double)i * step;
}

// What a sample does with a real time under a Lambda: getTau, the clamp of trajectory.h:69-70 / 101-102 (REFERENCE: to
// the SCALED total, as written; ROBUST: to taus[S]), Lambda::evaluate.  raw: getTau as it came.
template <class L>
MPLX_HD double sample_tau(const L &ld, int n, bool robust, double t, double total, double tau_end, double *raw, bool *found,
                          double *lam, double *lam_dot) {
  double tau;
  if (robust) {
    tau = get_tau_robust(ld, n, t, total, tau_end);
    *found = true;
  } else {
    tau = get_tau_reference(ld, n, t, found);
  }
  *raw = tau;
  const double hi = robust ? tau_end : total;
  if (tau < 0) tau = 0;
  if (tau > hi) tau = hi;
  lambda_eval(ld, n, tau, robust, lam, lam_dot);
  return tau;
}

// scale_down: the records of one axis of one segment (include/mplx_scale.h).  max_l == 0: nothing recorded yet.
struct DownRec {
  double max_l, t_lo, t_hi;
};

MPLX_HD void down_record(DownRec &r, double l, double t) {
  if (r.max_l == 0) {
    r.max_l = l;
    r.t_lo = t;
    r.t_hi = t;
    return;
  }
  r.max_l = l > r.max_l ? l : r.max_l;
  r.t_lo = t < r.t_lo ? t : r.t_lo;
  r.t_hi = t > r.t_hi ? t : r.t_hi;
}

// ORDER 1: velocity, l = |v| / lim; ORDER 2: acceleration, l = sqrt(|a| / lim).  tau0 = taus[s]; first: s == 0.
template <int ORDER>
MPLX_HD void down_axis(const double (&c)[6], double dt, double tau0, bool first, double lim, DownRec &r) {
  if (!(limits::axis_max<ORDER, true>(c, dt) > lim)) return;
  const limits::Roots ts = ORDER == 1 ? limits::solve<true>(c[0] / 6, c[1] / 2, c[2], c[3]) : limits::solve<true>(0.0, c[0] / 2, c[1], c[2]);
#pragma unroll
  for (int i = 0; i < 5; i++) {
    double tv;
    if (i < 3) {
      if (i >= ts.n) continue;
      tv = ts.r[i];
      if (!(tv > 0 && tv < dt)) continue;
    } else if (i == 3) {
      if (first) continue;
      tv = 0.0;
    } else {
      tv = dt;
    }
    const double x = fabs(limits::poly_x<ORDER>(c, tv));
    const double l = ORDER == 1 ? x / lim : sqrt(x / lim);
    if (l > 1) down_record(r, l, tau0 + tv);
  }
}

}  // namespace scale
}  // namespace mplx
#endif
