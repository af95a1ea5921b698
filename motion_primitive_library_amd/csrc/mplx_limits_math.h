// mplx_limits_math.h -- the root finder and the per-axis maxima of include/mplx_limits.h, written once for the device
// (limits_kernel.hip) and for a host build of the same expressions (MPLX_HD is empty without a HIP compiler).
//
// Reference: include/mpl_basis/math.h:21-66 (quad, cubic), 117-131 (solve), include/mpl_basis/primitive.h:134-145 (v, a,
// j), 152-193 (extrema_v / _a / _j), 353-394 (max_vel / max_acc / max_jrk).  Expression for expression, under
// -ffp-contract=off, power() as repeated multiplication.  ALL = false is the reference with its quirks; ALL = true looks
// at every root returned, clamps the acos argument and adds the jerk's true extremum (include/mplx_limits.h).
#ifndef MPLX_LIMITS_MATH_H
#define MPLX_LIMITS_MATH_H

#include <math.h>

#if defined(__HIPCC__)
#define MPLX_HD __host__ __device__ __forceinline__
#else
#define MPLX_HD inline
#endif

namespace mplx {
namespace limits {

struct Roots {
  double r[3];
  int n;
};

// math.h:22-32: b t^2 + c t + d = 0, both roots as written (for b < 0 the larger one comes first)
MPLX_HD Roots quad(double b, double c, double d) {
  Roots o{{0.0, 0.0, 0.0}, 0};
  const double p = c * c - 4 * b * d;
  if (p < 0) return o;
  o.r[0] = (-c - sqrt(p)) / (2 * b);
  o.r[1] = (-c + sqrt(p)) / (2 * b);
  o.n = 2;
  return o;
}

// math.h:35-66: a t^3 + b t^2 + c t + d = 0; a NaN discriminant takes the acos branch, as `else` does
template <bool ALL>
MPLX_HD Roots cubic(double a, double b, double c, double d) {
  Roots o{{0.0, 0.0, 0.0}, 0};
  const double a2 = b / a, a1 = c / a, a0 = d / a;
  const double Q = (3 * a1 - a2 * a2) / 9;
  const double R = (9 * a1 * a2 - 27 * a0 - 2 * a2 * a2 * a2) / 54;
  const double D = Q * Q * Q + R * R;
  if (D > 0) {
    const double S = cbrt(R + sqrt(D)), T = cbrt(R - sqrt(D));
    o.r[0] = -a2 / 3 + (S + T);
    o.n = 1;
  } else if (D == 0) {
    const double S = cbrt(R);
    o.r[0] = -a2 / 3 + S + S;
    o.r[1] = -a2 / 3 - S;
    o.n = 2;
  } else {
    double x = R / sqrt(-Q * Q * Q);
    if (ALL) x = x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x);
    const double theta = acos(x);
    o.r[0] = 2 * sqrt(-Q) * cos(theta / 3) - a2 / 3;
    o.r[1] = 2 * sqrt(-Q) * cos((theta + 2 * M_PI) / 3) - a2 / 3;
    o.r[2] = 2 * sqrt(-Q) * cos((theta + 4 * M_PI) / 3) - a2 / 3;
    o.n = 3;
  }
  return o;
}

// math.h:117-131 with a == 0: solve(0, b, c, d, e)
template <bool ALL>
MPLX_HD Roots solve(double b, double c, double d, double e) {
  if (b != 0) return cubic<ALL>(b, c, d, e);
  if (c != 0) return quad(c, d, e);
  Roots o{{0.0, 0.0, 0.0}, 0};
  if (d != 0) {
    o.r[0] = -e / d;
    o.n = 1;
  }
  return o;
}

// primitive.h:134-145, c = c(0) .. c(5)
MPLX_HD double poly_v(const double (&c)[6], double t) {
  const double t3 = (t * t) * t, t4 = t3 * t;
  return (((c[0] / 24 * t4 + c[1] / 6 * t3) + c[2] / 2 * t * t) + c[3] * t) + c[4];
}
MPLX_HD double poly_a(const double (&c)[6], double t) {
  const double t3 = (t * t) * t;
  return ((c[0] / 6 * t3 + c[1] / 2 * t * t) + c[2] * t) + c[3];
}
MPLX_HD double poly_j(const double (&c)[6], double t) { return (c[0] / 2 * t * t + c[1] * t) + c[2]; }

template <int ORDER>
MPLX_HD double poly_x(const double (&c)[6], double t) {
  return ORDER == 1 ? poly_v(c, t) : (ORDER == 2 ? poly_a(c, t) : poly_j(c, t));
}

// primitive.h:353-394 for ORDER = 1 (max_vel), 2 (max_acc), 3 (max_jrk) of one axis with duration t.  The scan of
// extrema_x (accept, `>= t` ends it, anything else is passed over) and the loop of max_x, which tests the accepted root
// again, are one loop here: the second test is the first.
template <int ORDER, bool ALL>
MPLX_HD double axis_max(const double (&c)[6], double t) {
  Roots ts{{0.0, 0.0, 0.0}, 0};
  if (ORDER == 1) {
    ts = solve<ALL>(c[0] / 6, c[1] / 2, c[2], c[3]);
  } else if (ORDER == 2) {
    ts = solve<ALL>(0.0, c[0] / 2, c[1], c[2]);
  } else if (c[0] != 0) {
    ts.r[0] = -c[1] * 2 / c[0];  // (as written, primitive.h:189: twice the time at which j' = c0 t + c1 vanishes)
    ts.n = 1;
    if (ALL) {  // ... so the true extremum is one more point to look at
      ts.r[1] = -c[1] / c[0];
      ts.n = 2;
    }
  }
  const double x0 = fabs(poly_x<ORDER>(c, 0.0)), xt = fabs(poly_x<ORDER>(c, t));
  double m = x0 < xt ? xt : x0;  // std::max
  bool ended = false;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if (i >= ts.n || ended) continue;
    const double it = ts.r[i];
    if (it > 0 && it < t) {
      const double x = fabs(poly_x<ORDER>(c, it));
      m = x > m ? x : m;
    } else if (it >= t) {
      ended = !ALL;
    }
  }
  return m;
}

}  // namespace limits
}  // namespace mplx
#endif
