"""The model the limits calls (include/mplx_limits.h) are compared with, its exact counterpart, and the inputs of their
tests.

A float64 restatement of math.h:21-66 (quad, cubic), 117-131 (solve) and primitive.h:152-193 (extrema_v / _a / _j),
353-394 (max_vel / max_acc / max_jrk), 450-496 (validate_primitive, validate_xxx), operation for operation, with
math.sqrt / acos / cos and numpy.cbrt (this Python has no math.cbrt); v / a / j are traj_model.poly_v / poly_a / poly_j.

Two modes.  REFERENCE is the reference with its quirks: of the roots solve() returns, in its order, `0 < r < t` is
accepted, `r >= t` ENDS the scan, anything else (negative, NaN) is passed over -- and quad (for b < 0) and the acos
branch of cubic return their LARGEST root first, so smaller roots inside (0, t) are often never looked at.  ALL_ROOTS
looks at every root returned, clamps the acos argument to [-1, 1], and for the jerk adds the true extremum -c1 / c0 to
the reference's -c1 * 2 / c0 (primitive.h:189 doubles the time).

truth_*: the same maxima from the exact roots (mpmath, 50 digits; the float coefficients taken as exact rationals)."""
import functools
import math

import numpy as np

import solve_model as SM
import traj_model as TM

REFERENCE, ALL_ROOTS = 0, 1
EXCEED_VEL, EXCEED_ACC, EXCEED_JRK = 1, 2, 4
F = np.float64
NAN = F(np.nan)
PI = F(math.pi)
POLY = {1: TM.poly_v, 2: TM.poly_a, 3: TM.poly_j}


def _sqrt(x):
    return F(math.sqrt(x)) if x >= 0 else NAN  # (a negative or NaN argument: NaN, where math.sqrt raises)


def _acos(x):
    return F(math.acos(x)) if -1 <= x <= 1 else NAN


def _cos(x):
    return F(math.cos(x)) if np.isfinite(x) else NAN


def quad(b, c, d):
    """math.h:22-32."""
    p = c * c - 4 * b * d
    if p < 0:
        return []
    return [(-c - _sqrt(p)) / (2 * b), (-c + _sqrt(p)) / (2 * b)]


def cubic(a, b, c, d, mode):
    """math.h:35-66."""
    a2, a1, a0 = b / a, c / a, d / a
    Q = (3 * a1 - a2 * a2) / 9
    R = (9 * a1 * a2 - 27 * a0 - 2 * a2 * a2 * a2) / 54
    D = Q * Q * Q + R * R
    if D > 0:
        S, T = np.cbrt(R + _sqrt(D)), np.cbrt(R - _sqrt(D))
        return [-a2 / 3 + (S + T)]
    if D == 0:
        S = np.cbrt(R)
        return [-a2 / 3 + S + S, -a2 / 3 - S]
    x = R / _sqrt(-Q * Q * Q)
    if mode == ALL_ROOTS:
        x = F(-1.0) if x < -1 else (F(1.0) if x > 1 else x)
    theta = _acos(x)
    return [2 * _sqrt(-Q) * _cos(theta / 3) - a2 / 3, 2 * _sqrt(-Q) * _cos((theta + 2 * PI) / 3) - a2 / 3,
            2 * _sqrt(-Q) * _cos((theta + 4 * PI) / 3) - a2 / 3]


def solve(b, c, d, e, mode):
    """math.h:117-131 with a == 0: solve(0, b, c, d, e)."""
    if b != 0:
        return cubic(b, c, d, e, mode)
    if c != 0:
        return quad(c, d, e)
    if d != 0:
        return [-e / d]
    return []


def extrema(c, order, mode):
    """The roots extrema_v / _a / _j look at, in the order solve returns them (primitive.h:152-193)."""
    c = [F(x) for x in c]
    with np.errstate(all="ignore"):
        if order == 1:
            return solve(c[0] / 6, c[1] / 2, c[2], c[3], mode)
        if order == 2:
            return solve(F(0.0), c[0] / 2, c[1], c[2], mode)
        if c[0] == 0:
            return []
        # primitive.h:189 as written: twice the time at which j' = c0 t + c1 vanishes; ALL_ROOTS adds the true extremum
        return [-c[1] * 2 / c[0]] + ([-c[1] / c[0]] if mode == ALL_ROOTS else [])


def accepted(roots, t, mode):
    out = []
    for it in roots:
        if it > 0 and it < t:
            out.append(it)
        elif it >= t and mode == REFERENCE:
            break
    return out


def axis_max(c, t, order, mode, want_roots=False):
    """primitive.h:353-394 for one axis: max_vel (order 1), max_acc (2), max_jrk (3)."""
    c, t = np.asarray(c, dtype=F), F(t)
    roots = extrema(c, order, mode)
    ts = accepted(roots, t, mode)
    with np.errstate(all="ignore"):
        x0, xt = abs(POLY[order](c, F(0.0))), abs(POLY[order](c, t))
        m = xt if x0 < xt else x0  # std::max
        for it in ts:
            x = abs(POLY[order](c, it))
            m = x if x > m else m
    return (m, roots, ts) if want_roots else m


def checks_of(control):
    """validate_primitive, primitive.h:450-475: which of vel / acc / jrk the control checks."""
    o = int(control) & 0x0F
    return [o >= 0x03, o >= 0x07, o >= 0x0F]


def traj_limits(coefs, dts, control, mv, ma, mj, mode):
    """coefs: per segment [D][6]; dts [S].  What mplx_poly_limits returns for one trajectory."""
    D = len(coefs[0])
    lim = [F(mv), F(ma), F(mj)]
    chk = [c and not (l <= 0) for c, l in zip(checks_of(control), lim)]
    m = np.zeros((3, D))
    first_bad = -1
    for s, (cs, t) in enumerate(zip(coefs, dts)):
        ok = True
        for q in range(3):
            for i in range(D):
                x = axis_max(cs[i], t, q + 1, mode)
                m[q, i] = x if (s == 0 or x > m[q, i]) else m[q, i]
                if chk[q] and x > lim[q]:
                    ok = False
        if not ok and first_bad < 0:
            first_bad = s
    exceed = 0
    for q in range(3):
        top = m[q, 0]
        for i in range(1, D):
            top = m[q, i] if m[q, i] > top else top
        if not (lim[q] <= 0) and top > lim[q]:
            exceed |= 1 << q
    return {"max_vel": m[0], "max_acc": m[1], "max_jrk": m[2], "exceed": exceed, "valid": int(first_bad < 0), "first_bad": first_bad}


# ------------------------------------------------------------------------------------------------------------ truth
def _mp():
    import mpmath
    mpmath.mp.dps = 50
    return mpmath


def _mp_poly(c, order):
    """Coefficients, highest power first, of v / a / j as exact values."""
    mp = _mp()
    c = [mp.mpf(float(x)) for x in c]
    if order == 1:
        return [c[0] / 24, c[1] / 6, c[2] / 2, c[3], c[4]]
    if order == 2:
        return [c[0] / 6, c[1] / 2, c[2], c[3]]
    return [c[0] / 2, c[1], c[2]]


def _mp_eval(p, t):
    r = _mp().mpf(0)
    for a in p:
        r = r * t + a
    return r


def true_roots(c, order):
    """Every real root of the derivative of v / a / j (order 1 / 2 / 3), exact to 50 digits."""
    mp = _mp()
    p = _mp_poly(c, order)
    n = len(p) - 1
    d = [a * (n - i) for i, a in enumerate(p[:-1])]
    while d and d[0] == 0:
        d = d[1:]
    if len(d) < 2:
        return []
    roots = mp.polyroots(d, maxsteps=500, extraprec=400)
    return [mp.re(r) for r in roots if abs(mp.im(r)) <= mp.mpf(10) ** -30 * (1 + abs(r))]


def scale_of(c, t, order):
    """sum_j |term_j| of the evaluated polynomial at t."""
    mp = _mp()
    p = _mp_poly(c, order)
    t = mp.mpf(float(t))
    n = len(p) - 1
    return float(sum(abs(a * t ** (n - i)) for i, a in enumerate(p)))


def truth_all(c, t, order):
    """max |x| over {0, t} and every true root in (0, t)."""
    mp = _mp()
    p, tt = _mp_poly(c, order), mp.mpf(float(t))
    pts = [mp.mpf(0), tt] + [r for r in true_roots(c, order) if 0 < r < tt]
    return max(abs(_mp_eval(p, x)) for x in pts)


def truth_reference(c, t, order, accepted_roots):
    """max |x| over {0, t} and, for each root the float model accepted, the nearest true root.  The reference's jerk
    "root" -c1 * 2 / c0 is no root of anything: for order 3 the point is that expression's exact value."""
    mp = _mp()
    p, tt = _mp_poly(c, order), mp.mpf(float(t))
    tr = true_roots(c, order)
    pts = [mp.mpf(0), tt]
    for it in accepted_roots:
        if order == 3:
            pts.append(-mp.mpf(float(c[1])) * 2 / mp.mpf(float(c[0])))
        else:
            pts.append(min(tr, key=lambda r: abs(r - mp.mpf(float(it)))))
    return max(abs(_mp_eval(p, x)) for x in pts)


def err(x, truth):
    """|x - truth| with the difference formed exactly, rounded once."""
    return float(abs(_mp().mpf(float(x)) - truth))


# ----------------------------------------------------------------------------------------------------------- inputs
N_QUINTICS = 400


@functools.lru_cache(maxsize=None)
def quintics():
    """400 seeded JRK two-point quintics on one axis: end states uniform in +-2 / +-1.5 / +-1 for pos / vel / acc, T in
    [0.4, 3], coefficients from the exact solve rounded once: (coef [400][6] as c(0) .. c(5), T [400])."""
    rng = np.random.default_rng(20240607)
    coef, Ts = np.zeros((N_QUINTICS, 6)), np.zeros(N_QUINTICS)
    flags = np.full(2, 7, np.uint8)
    for n in range(N_QUINTICS):
        vals = np.zeros((3, 2, 1))
        vals[0, :, 0] = rng.uniform(-2, 2, 2)
        vals[1, :, 0] = rng.uniform(-1.5, 1.5, 2)
        vals[2, :, 0] = rng.uniform(-1, 1, 2)
        T = rng.uniform(0.4, 3.0)
        p = SM.to_float(SM.solve_exact(vals, flags, np.array([T]), 2))
        coef[n] = SM.to_primitive_coeffs(p, 2)[0, 0]
        Ts[n] = T
    return coef, Ts


@functools.lru_cache(maxsize=None)
def quintic_reference():
    """Per quintic, mode and order 1 .. 3: dict(model, truth, e_ref, scale, near) -- near: a root the model computed lies
    within 2^-30 T of 0 or T, where acceptance could flip between two libraries.  Computed once, shared."""
    coef, Ts = quintics()
    out = []
    for c, t in zip(coef, Ts):
        row = {}
        for mode in (REFERENCE, ALL_ROOTS):
            for order in (1, 2, 3):
                m, roots, ts = axis_max(c, t, order, mode, want_roots=True)
                truth = truth_reference(c, t, order, ts) if mode == REFERENCE else truth_all(c, t, order)
                near = any(abs(r) <= 2.0 ** -30 * t or abs(r - t) <= 2.0 ** -30 * t for r in roots if np.isfinite(r))
                row[(mode, order)] = {"model": float(m), "truth": truth, "e_ref": err(m, truth),
                                      "scale": scale_of(c, t, order), "near": near}
        out.append(row)
    return out
