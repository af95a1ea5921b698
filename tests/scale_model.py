"""The model the time-scaling calls (include/mplx_scale.h) are compared with, its exact counterpart, and the inputs of
their tests.

A float64 restatement of lambda.h (LambdaSeg, Lambda::getT / getTau / evaluate), math.h:69-131 (quartic, the five-argument
solve), trajectory.h:99-160 (evaluate under a Lambda, scale) and of this library's own parts -- the Hermite coefficients,
the ROBUST checks and inverse, scale_down -- operation for operation as csrc/mplx_scale_math.h states them; quad and the
lower branches of solve are limits_model's, cubic is restated here with the C library's cbrt.

REFERENCE is the reference with its quirks (the 1e-5 clamp of the coefficients, a getTau that returns -1 where the
closed-form quartic gives no root inside the segment, the clamp of tau to the SCALED total); ROBUST validates the points,
applies no clamp, and inverts the time map by LAMBDA_NEWTON Newton steps from the closed-form root.

exact_*: the same quantities in rational arithmetic (fractions.Fraction; the float inputs taken as exact)."""
import functools
from fractions import Fraction

import numpy as np

import limits_model as LM
import traj_model as TM

REFERENCE, ROBUST = 0, 1
BAD_POINTS, NOT_POSITIVE = 32, 64
MAX_SEGS, NEWTON = 8, 3
F = np.float64
INF = F(np.inf)
EPS = 2.0 ** -52


def _isnan(x):
    return x != x


def _libm_cbrt():
    """The C library's cbrt, which the reference's std::cbrt is: numpy.cbrt is another implementation and differs from it
    in the last bit often enough to move a root of the quartic across the end of its segment."""
    import ctypes
    import ctypes.util
    try:
        fn = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").cbrt
        fn.restype, fn.argtypes = ctypes.c_double, [ctypes.c_double]
        return lambda x: F(fn(float(x)))
    except (OSError, AttributeError):
        return np.cbrt


_cbrt = _libm_cbrt()


def cubic(a, b, c, d):
    """math.h:35-66, as limits_model.cubic in REFERENCE mode, with the C library's cbrt."""
    a2, a1, a0 = b / a, c / a, d / a
    Q = (3 * a1 - a2 * a2) / 9
    R = (9 * a1 * a2 - 27 * a0 - 2 * a2 * a2 * a2) / 54
    D = Q * Q * Q + R * R
    if D > 0:
        S, T = _cbrt(R + LM._sqrt(D)), _cbrt(R - LM._sqrt(D))
        return [-a2 / 3 + (S + T)]
    if D == 0:
        S = _cbrt(R)
        return [-a2 / 3 + S + S, -a2 / 3 - S]
    theta = LM._acos(R / LM._sqrt(-Q * Q * Q))
    return [2 * LM._sqrt(-Q) * LM._cos(theta / 3) - a2 / 3, 2 * LM._sqrt(-Q) * LM._cos((theta + 2 * LM.PI) / 3) - a2 / 3,
            2 * LM._sqrt(-Q) * LM._cos((theta + 4 * LM.PI) / 3) - a2 / 3]


def quartic(a, b, c, d, e):
    """math.h:69-110: [(root, ...)] in the reference's order."""
    a3, a2, a1, a0 = b / a, c / a, d / a, e / a
    ys = cubic(F(1.0), -a2, a1 * a3 - 4 * a0, 4 * a2 * a0 - a1 * a1 - a3 * a3 * a0)
    y1 = ys[0]
    r = a3 * a3 / 4 - a2 + y1
    if r < 0:
        return []
    R = LM._sqrt(r)
    if R != 0:
        D = LM._sqrt(0.75 * a3 * a3 - R * R - 2 * a2 + 0.25 * (4 * a3 * a2 - 8 * a1 - a3 * a3 * a3) / R)
        E = LM._sqrt(0.75 * a3 * a3 - R * R - 2 * a2 - 0.25 * (4 * a3 * a2 - 8 * a1 - a3 * a3 * a3) / R)
    else:
        D = LM._sqrt(0.75 * a3 * a3 - 2 * a2 + 2 * LM._sqrt(y1 * y1 - 4 * a0))
        E = LM._sqrt(0.75 * a3 * a3 - 2 * a2 - 2 * LM._sqrt(y1 * y1 - 4 * a0))
    out = []
    if not _isnan(D):
        out += [-a3 / 4 + R / 2 + D / 2, -a3 / 4 + R / 2 - D / 2]
    if not _isnan(E):
        out += [-a3 / 4 - R / 2 + E / 2, -a3 / 4 - R / 2 - E / 2]
    return out


def solve5(a, b, c, d, e):
    """math.h:117-131.  Also returns whether the result passed through cbrt / acos / cos (anything above quad)."""
    if a != 0:
        return quartic(a, b, c, d, e), True
    if b != 0:
        return cubic(b, c, d, e), True
    return LM.solve(b, c, d, e, LM.REFERENCE), False


def seg_getT(a, t):
    t3 = (t * t) * t
    t4 = t3 * t
    return ((a[0] / 4 * t4 + a[1] / 3 * t3) + a[2] / 2 * t * t) + a[3] * t


def seg_lambda(a, tau):
    t3 = (tau * tau) * tau
    return ((a[0] * t3 + a[1] * tau * tau) + a[2] * tau) + a[3]


def seg_lambda_dot(a, tau):
    return (3 * a[0] * tau * tau + 2 * a[1] * tau) + a[2]


def hermite(p1, v1, t1, p2, v2, t2):
    """The stated expression tree of include/mplx_scale.h: a3 a2 a1 a0 in absolute virtual time."""
    h = t2 - t1
    m = (p2 - p1) / h
    c3 = ((v1 + v2) - 2 * m) / (h * h)
    c2 = ((3 * m - 2 * v1) - v2) / h
    return [c3, c2 - 3 * c3 * t1, (v1 - 2 * c2 * t1) + 3 * c3 * t1 * t1, ((p1 - v1 * t1) + c2 * t1 * t1) - c3 * t1 * t1 * t1]


def seg_from_a(a, t1, t2):
    """The 8 fields of a segment from its (clamped or not) coefficients: lambda.h:43-46."""
    a = [F(x) for x in a]
    g0 = seg_getT(a, t1)
    return np.array(a + [t1, t2, g0, seg_getT(a, t2) - g0], dtype=F)


def build_seg(p1, v1, t1, p2, v2, t2, mode):
    """(the 8 fields a3 a2 a1 a0 ti tf getT(ti) dT, status bits), csrc/mplx_scale_math.h build_seg."""
    p1, v1, t1, p2, v2, t2 = (F(x) for x in (p1, v1, t1, p2, v2, t2))
    with np.errstate(all="ignore"):
        a = hermite(p1, v1, t1, p2, v2, t2)
        if mode == REFERENCE:
            a = [F(0.0) if abs(x) < 1e-5 else x for x in a]
        seg = seg_from_a(a, t1, t2)
        if not np.isfinite([p1, v1, t1, p2, v2, t2]).all():
            return seg, BAD_POINTS
        if mode == REFERENCE:
            return seg, 0
        if not (t2 > t1) or not (p1 > 0) or not (p2 > 0):
            return seg, BAD_POINTS
        pos = seg_lambda(a, t1) > 0 and seg_lambda(a, t2) > 0
        ts = []
        if 3 * a[0] != 0:
            ts = LM.quad(3 * a[0], 2 * a[1], a[2])
        elif 2 * a[1] != 0:
            ts = [-a[2] / (2 * a[1])]
        for r in ts:
            if r > t1 and r < t2 and not (seg_lambda(a, r) > 0):
                pos = False
    return seg, (0 if pos else NOT_POSITIVE)


class Lambda:
    """segs [n][8]; mode."""

    def __init__(self, segs, mode):
        self.segs, self.mode, self.n = np.asarray(segs, dtype=F).reshape(-1, 8), mode, len(segs)

    def getT(self, tau):
        """lambda.h:127-138."""
        tau, T = F(tau), F(0.0)
        with np.errstate(all="ignore"):
            for s in self.segs:
                if tau >= s[4] and tau <= s[5]:
                    return T + (seg_getT(s[:4], tau) - s[6])
                T = T + s[7]
        return T

    def evaluate(self, tau):
        """lambda.h:116-125: (lambda, lambda_dot)."""
        tau = F(tau)
        pick = None
        for s in self.segs:
            if tau >= s[4] and tau < s[5]:
                pick = s
                break
        if pick is None:
            if self.mode == REFERENCE:
                return F(0.0), F(0.0)
            pick = self.segs[-1]
        with np.errstate(all="ignore"):
            return seg_lambda(pick[:4], tau), seg_lambda_dot(pick[:4], tau)

    def total(self):
        T = F(0.0)
        for s in self.segs:
            T = T + s[7]
        return T

    def get_tau_reference(self, t, want_info=False):
        """lambda.h:140-161: (tau, found); want_info: also (segment, libm) -- libm: the roots came through cbrt / acos / cos."""
        t, T = F(t), F(0.0)
        with np.errstate(all="ignore"):
            for n, s in enumerate(self.segs):
                dT = s[7]
                if t >= T and t <= T + dT:
                    ts, libm = solve5(s[0] / 4, s[1] / 3, s[2] / 2, s[3], T - t - s[6])
                    for it in ts:
                        if it >= s[4] and it <= s[5]:
                            return (it, True, n, libm) if want_info else (it, True)
                T = T + dT
        return (F(-1.0), False, -1, False) if want_info else (F(-1.0), False)

    def robust_segment(self, t):
        t, T0, s = F(t), F(0.0), 0
        while s < self.n - 1:
            dT = self.segs[s][7]
            if t <= T0 + dT:
                break
            T0 = T0 + dT
            s += 1
        return s, T0

    def get_tau_robust(self, t, total, tau_end, newton=NEWTON):
        t = F(t)
        if not (t > 0):
            return F(0.0)
        if t >= total:
            return F(tau_end)
        n, T0 = self.robust_segment(t)
        s = self.segs[n]
        a, ti, tf, g0, dT = s[:4], s[4], s[5], s[6], s[7]
        with np.errstate(all="ignore"):
            ts, _ = solve5(a[0] / 4, a[1] / 3, a[2] / 2, a[3], T0 - t - g0)
            best, dist = ti + (t - T0) / dT * (tf - ti), INF
            for r in ts:
                d = ti - r if r < ti else (r - tf if r > tf else (F(0.0) if r == r else INF))
                if d < dist:
                    dist, best = d, r
            tau = best if best >= ti else ti
            tau = tf if tau > tf else tau
            for _ in range(newton):
                step = ((seg_getT(a, tau) - g0) + T0 - t) / seg_lambda(a, tau)
                if abs(step) < INF:
                    tau = tau - step
                tau = tau if tau >= ti else ti
                tau = tf if tau > tf else tau
        return tau

    def sample_tau(self, t, total, tau_end):
        """What a sample does with the real time t: (tau clamped, raw getTau, found, lambda, lambda_dot)."""
        if self.mode == ROBUST:
            raw, found = self.get_tau_robust(t, total, tau_end), True
        else:
            raw, found = self.get_tau_reference(t)
        tau, lam, dot = self.clamp_eval(raw, total, tau_end)
        return tau, raw, found, lam, dot

    def clamp_eval(self, raw, total, tau_end):
        """trajectory.h:69-70 / 101-102 (REFERENCE: the scaled total) and Lambda::evaluate at the clamped tau."""
        hi = F(tau_end) if self.mode == ROBUST else F(total)
        tau = F(raw)
        if tau < 0:
            tau = F(0.0)
        if tau > hi:
            tau = hi
        lam, dot = self.evaluate(tau)
        return tau, lam, dot


def build_lambda(p, v, t, mode):
    """Lambda(vs): (Lambda or None, status) from the point lists p, v, t."""
    n = len(p)
    if n < 2 or n > 9:
        return None, BAD_POINTS
    segs, status = [], 0
    for j in range(n - 1):
        seg, st = build_seg(p[j], v[j], t[j], p[j + 1], v[j + 1], t[j + 1], mode)
        segs.append(seg)
        status |= st
    if status & BAD_POINTS:
        status = BAD_POINTS
    return (None, status) if status else (Lambda(segs, mode), 0)


def scale_points(ri, rf, T):
    """trajectory.h:140-153; None for a ratio that is <= 0 or not finite."""
    ri, rf = F(ri), F(rf)
    if not (ri > 0 and rf > 0 and np.isfinite(ri) and np.isfinite(rf)):
        return None
    with np.errstate(all="ignore"):
        return [F(1.0) / ri, F(1.0) / rf], [F(0.0), F(0.0)], [F(0.0), F(T)]


def scale(taus, ri, rf, mode):
    """Trajectory::scale: dict(lam, status, Ts, total)."""
    pts = scale_points(ri, rf, taus[-1])
    lam, status = (None, BAD_POINTS) if pts is None else build_lambda(*pts, mode)
    return with_Ts(lam, status, taus)


def with_Ts(lam, status, taus):
    if lam is None:
        return {"lam": None, "status": status, "Ts": None, "total": None}
    Ts = np.array([lam.getT(x) for x in taus], dtype=F)
    return {"lam": lam, "status": 0, "Ts": Ts, "total": Ts[-1]}


# ---------------------------------------------------------------------------------------------------- scale_down
def down_axis(c, dt, tau0, first, lim, order, rec):
    """One axis of one segment: rec = [max_l, t_lo, t_hi] or None, updated in the device's order."""
    c, dt, lim = np.asarray(c, dtype=F), F(dt), F(lim)
    if not (LM.axis_max(c, dt, order, LM.ALL_ROOTS) > lim):
        return rec
    with np.errstate(all="ignore"):
        cands = [r for r in LM.extrema(c, order, LM.ALL_ROOTS)[:3] if r > 0 and r < dt]
        if not first:
            cands.append(F(0.0))
        cands.append(dt)
        for tv in cands:
            x = abs(LM.POLY[order](c, tv))
            l = x / lim if order == 1 else LM._sqrt(x / lim)
            if l > 1:
                rec = record(rec, l, F(tau0) + tv)
    return rec


def record(rec, l, t):
    if rec is None:
        return [l, t, t]
    return [l if l > rec[0] else rec[0], t if t < rec[1] else rec[1], t if t > rec[2] else rec[2]]


def scale_down(coefs, dts, taus, mv, ma, ri, rf, mode):
    """coefs: per segment [D][6].  dict(scaled, max_l, t_lo, t_hi, points, lam, status, Ts, total)."""
    rec = None
    for s, (cs, dt) in enumerate(zip(coefs, dts)):
        seg = None
        for c in cs:
            if mv > 0:
                seg = down_axis(c, dt, taus[s], s == 0, mv, 1, seg)
            if ma > 0:
                seg = down_axis(c, dt, taus[s], s == 0, ma, 2, seg)
        if seg is not None:
            rec = record(record(rec, seg[0], seg[1]), seg[0], seg[2])
    if rec is None:
        return {"scaled": 0}
    max_l, t_lo, t_hi = rec
    T = F(taus[-1])
    pi, pf = (max_l if ri <= 0 else F(ri)), (max_l if rf <= 0 else F(rf))
    p, t = [pi, max_l], [F(0.0), t_lo]
    if t_hi > t_lo:
        p.append(max_l)
        t.append(t_hi)
    if T > t_hi:
        p.append(pf)
        t.append(T)
    lam, status = build_lambda(p, [F(0.0)] * len(p), t, mode)
    out = {"scaled": 1, "max_l": max_l, "t_lo": t_lo, "t_hi": t_hi, "points": (p, t)}
    out.update(with_Ts(lam, status, taus))
    return out


# ------------------------------------------------------------------------------------------------------- samples
def sample_rows(coef, coef_yaw, taus, tau, lam, lam_dot, time, command):
    """The rows of one sample at the (clamped) virtual time tau: trajectory.h:67-135 with the given lambda, lambda_dot.
    coef [S][D][6], coef_yaw [S][6], taus [S + 1]."""
    S, D = len(coef), len(coef[0])
    tau = F(tau)
    seg = S - 1  # (also for a Command whose tau lies past taus[S]: the device's bisection ends there)
    for i in range(S):
        if tau >= taus[i] and (tau <= taus[i + 1] if command else tau < taus[i + 1]):
            seg = i
            break
    t = tau - taus[seg]
    rows = np.zeros(4 * D + (3 if command else 1))
    with np.errstate(all="ignore"):
        for i in range(D):
            c = np.asarray(coef[seg][i], dtype=F)
            p, v, a, j = TM.poly_p(c, t), TM.poly_v(c, t), TM.poly_a(c, t), TM.poly_j(c, t)
            if command:
                vel = v / lam
                acc = a / lam / lam - vel * lam_dot / lam / lam / lam
                l3 = (F(1.0) * lam) * lam * lam
                l4 = l3 * lam
                jrk = j / lam / lam - 3 / l3 * acc * acc * lam_dot + 3 / l4 * vel * lam_dot * lam_dot
            else:
                vel, acc, jrk = v, a, j
            rows[i], rows[D + i], rows[2 * D + i], rows[3 * D + i] = p, vel, acc, jrk
        cy = np.asarray(coef_yaw[seg], dtype=F)
        rows[4 * D] = TM.normalize_angle(TM.poly_p(cy, t))
        if command:
            rows[4 * D + 1] = TM.normalize_angle(TM.poly_v(cy, t))
            rows[4 * D + 2] = time
    return rows


# --------------------------------------------------------------------------------------------------------- exact
def _fr(x):
    return Fraction(float(x))


def exact_hermite(p1, v1, t1, p2, v2, t2):
    """The Hermite cubic through the two points in exact arithmetic: a3 a2 a1 a0 as Fractions."""
    p1, v1, t1, p2, v2, t2 = (_fr(x) for x in (p1, v1, t1, p2, v2, t2))
    h = t2 - t1
    m = (p2 - p1) / h
    c3 = (v1 + v2 - 2 * m) / (h * h)
    c2 = (3 * m - 2 * v1 - v2) / h
    return [c3, c2 - 3 * c3 * t1, v1 - 2 * c2 * t1 + 3 * c3 * t1 * t1, p1 - v1 * t1 + c2 * t1 * t1 - c3 * t1 ** 3]


def exact_getT(a, t):
    a, t = [_fr(x) if not isinstance(x, Fraction) else x for x in a], (t if isinstance(t, Fraction) else _fr(t))
    return a[0] / 4 * t ** 4 + a[1] / 3 * t ** 3 + a[2] / 2 * t * t + a[3] * t


def exact_tau(seg, T0, t, bits=100, near=None):
    """The root of getT(tau) - getT(ti) + T0 - t of one segment (its 8 float fields taken as exact), by rational bisection
    to (tf - ti) 2^-bits.  near=None: the root in [ti, tf], the cubic followed 2^-20 (tf - ti) past either end only where
    the segment itself holds no sign change (a time equal to the float total has its root there when the float total is
    not the exact one).  near=x: the root next to x -- a bracket around x, widened until the sign changes -- for a Lambda
    that is not positive (the reference's clamp makes such), whose time map has several.  None: no sign change."""
    a = [_fr(x) for x in seg[:4]]
    ti, tf = _fr(seg[4]), _fr(seg[5])
    base = _fr(T0) - _fr(t) - exact_getT(a, ti)

    def g(x):
        return exact_getT(a, x) + base

    def bracket():
        if near is not None:
            w = (tf - ti) / 2 ** 44
            while w < 4 * (tf - ti):
                lo, hi = _fr(near) - w, _fr(near) + w
                if (g(lo) > 0) != (g(hi) > 0) or g(lo) == 0 or g(hi) == 0:
                    return lo, hi
                w *= 4
            return None
        for pad in (0, (tf - ti) / 2 ** 20):
            lo, hi = ti - pad, tf + pad
            if (g(lo) > 0) != (g(hi) > 0) or g(lo) == 0 or g(hi) == 0:
                return lo, hi
        return None

    b = bracket()
    if b is None:
        return None
    lo, hi = b
    glo, ghi = g(lo), g(hi)
    if glo == 0:
        return lo
    if ghi == 0:
        return hi
    for _ in range(bits):
        mid = (lo + hi) / 2
        gm = g(mid)
        if gm == 0:
            return mid
        if (gm > 0) == (glo > 0):
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def err(x, truth):
    """|x - truth| with the difference formed exactly, rounded once."""
    return float(abs(_fr(x) - truth))


# -------------------------------------------------------------------------------------------------------- inputs
N_SWEEP, SWEEP_TIMES = 2000, 25


@functools.lru_cache(maxsize=None)
def sweep():
    """2 000 seeded scale(ri, rf) calls: (T [n], ri [n], rf [n]); T log-uniform in [0.5, 80], ratios log-uniform in
    [0.25, 4], every 40th call with ri == rf (the linear branch of solve)."""
    rng = np.random.default_rng(20240917)
    T = np.exp(rng.uniform(np.log(0.5), np.log(80.0), N_SWEEP))
    ri = np.exp(rng.uniform(np.log(0.25), np.log(4.0), N_SWEEP))
    rf = np.exp(rng.uniform(np.log(0.25), np.log(4.0), N_SWEEP))
    rf[::40] = ri[::40]
    return T, ri, rf


def sweep_times(total):
    """25 real times of one scaled trajectory, the ends included: i * (total / 24) for i < 24, then total itself (24 *
    (total / 24) can fall an ulp short of it)."""
    step = F(total) / F(SWEEP_TIMES - 1)
    return [F(i) * step for i in range(SWEEP_TIMES - 1)] + [F(total)]


def crafted_quintic(peak_v, T):
    """One axis whose velocity is v(t) = peak_v * 16 (t / T)^2 (1 - t / T)^2: zero at both ends with zero acceleration
    there, its single peak peak_v at t = T / 2, and |a| peaks of 16 peak_v / (3 sqrt(3) T) at T (1/2 -+ 1/(2 sqrt 3)).  Returns c(0) .. c(5) (primitive.h:128-131: v = c0/24 t^4 + c1/6 t^3 + c2/2 t^2 + c3 t + c4)."""
    k = 16.0 * peak_v
    return np.array([24 * k / T ** 4, -12 * k / T ** 3, 2 * k / T ** 2, 0.0, 0.0, 0.0])
