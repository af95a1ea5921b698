"""The models the trajectory solver (include/mplx_solve.h) is compared with, and the inputs of its tests.

Why a model and not the reference's own binary: the solver of the reference (mpl_traj_solver) needs Eigen's
partialPivLu, block and topRows; no Eigen exists on the build machine, oracle/stub_include has none of the three, and
oracle/ is frozen.  The reference's program therefore cannot be compiled, and two restatements stand in for it (a third
function restates the device, not the reference):

  solve_dense   src/mpl_traj_solver/poly_solver.cpp:23-221 line for line in float64: A, Q, the permutation table, M,
                A^-1 M, R, Rpp / Rpf, Dp, and the per-segment solve.  lu_solve below stands in for
                partialPivLu().solve: LU with partial pivoting (the first largest entry of a column, so equal pivots do
                not swap), multipliers and back substitution by true division.  It is written out rather than taken from
                numpy.linalg.solve because LAPACK builds differ in the last bit (some multiply by the reciprocal of a
                pivot), and the so = 0 results are compared bit for bit.  One stated deviation, as in the header: two
                waypoints with free end derivatives are solved (poly_solver.cpp:202-209 reads uninitialised memory).
  solve_exact   the same statement in fractions.Fraction with dense Gaussian elimination.  The inputs are doubles, hence
                exact rationals: this is the exact minimiser, and the yardstick of both solve_dense and the device.

  solve_block   not a model of the reference but a twin of the device: csrc/solve_kernel.hip's block elimination restated
                in float64 in the kernel's own operation order, so that the device's coefficients for so >= 1 can be held
                bit for bit.  It shares the kernel's derivation; solve_exact and solve_dense stay the yardstick of both.

plus allocate_time (traj_solver.h:122-130), setTime (poly_traj.cpp:64-69), toPrimitives (poly_traj.cpp:72-88), and the
six-coefficient primitive through tests/traj_model.py (poly_p / poly_v / poly_a / poly_j / effort_1d), class PolySet
being the Trajectory that traj_model.traverse and its evaluate walk.

A waypoint set is (vals, flags): vals [h_max = 3][W][D] float64 (pos, vel, acc) and flags [W] with use_pos 1, use_vel 2,
use_acc 4 (waypoint.h:43-50)."""
from fractions import Fraction

import numpy as np

import traj_model as tm

USE_POS, USE_VEL, USE_ACC = 1, 2, 4
VEL, ACC, JRK = 0x01, 0x03, 0x07
S_EMPTY, S_BAD_TIME, S_SINGULAR = 1, 2, 8
FACT = [1, 1, 2, 6, 24, 120]


def so_of(control):
    return {1: 0, 3: 1, 7: 2}[control & 0x0F]


def path_flags(W, so):
    """setPath (traj_solver.h:55-70): interior waypoints Control::VEL (position only), the ends the solver's control."""
    f = np.full(W, USE_POS, np.uint8)
    end = [USE_POS, USE_POS | USE_VEL, USE_POS | USE_VEL | USE_ACC][so]
    if W > 0:
        f[0] = f[-1] = end
    return f


def allocate_time(pos, v):
    """traj_solver.h:122-130: pos [W][D]; dts[s] = |pos[s+1] - pos[s]|_inf / v, or [] (W < 2 or v <= 0)."""
    pos = np.asarray(pos, dtype=np.float64)
    if len(pos) < 2 or not v > 0:
        return np.zeros(0)
    return np.array([np.max(np.abs(pos[i] - pos[i - 1])) / np.float64(v) for i in range(1, len(pos))], dtype=np.float64)


def set_time(dts):
    """poly_traj.cpp:64-69."""
    taus = [np.float64(0.0)]
    for t in dts:
        taus.append(taus[-1] + np.float64(t))
    return np.array(taus, dtype=np.float64)


def _power(t, n, one):
    r = one
    for _ in range(n):
        r = r * t
    return r


def _system(W, dts, so, flags, num):
    """poly_solver.cpp:37-167 with numbers made by `num` (np.float64 or Fraction): A, Q (lists of rows), the permutation
    table, n_fixed."""
    N, R, S, h = 2 * (so + 1), so + 1, W - 1, so + 1
    zero, one = num(0), num(1)
    A = [[zero] * (S * N) for _ in range(S * N)]
    Q = [[zero] * (S * N) for _ in range(S * N)]
    for i in range(S):
        T = num(dts[i])
        for n in range(N):
            if n < h:
                val = 1
                for m in range(n):
                    val *= n - m
                A[i * N + n][i * N + n] = num(val)
            for r in range(h):
                if r <= n:
                    val = 1
                    for m in range(r):
                        val *= n - m
                    A[i * N + h + r][i * N + n] = num(val) * _power(T, n - r, one)
            for r in range(N):
                if r >= R and n >= R:
                    val = 1
                    for m in range(R):
                        val *= (r - m) * (n - m)
                    e = r + n - 2 * R + 1
                    Q[i * N + r][i * N + n] = num(val) * _power(T, e, one) / num(e)
    n_fixed = sum(1 for w in range(W) for k in range(h) if flags[w] & (1 << k))
    table = []
    raw = fix = free = 0
    for w in range(W):
        inner = 0 < w < W - 1
        for k in range(h):
            if flags[w] & (1 << k):
                new = fix
                fix += 1
            else:
                new = n_fixed + free
                free += 1
            table.append((raw, new))
            if inner:
                table.append((raw + h, new))
            raw += 1
        if inner:
            raw += h
    return A, Q, table, n_fixed


def _fixed_rows(table, n_fixed, vals, N, D, num):
    h = N // 2
    Df = [[num(0)] * D for _ in range(n_fixed)]
    for raw, new in table:
        if new < n_fixed:
            w, k = (raw + h) // N, raw % h
            Df[new] = [num(vals[k][w][i]) for i in range(D)]
    return Df


def lu_solve(A, B):
    """X with A X = B by LU with partial pivoting in float64, one IEEE operation at a time."""
    a = np.array(A, dtype=np.float64)
    x = np.array(B, dtype=np.float64)
    if x.ndim == 1:
        return lu_solve(a, x[:, None])[:, 0]
    n = len(a)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(a[c:, c])))
        if piv != c:
            a[[c, piv]] = a[[piv, c]]
            x[[c, piv]] = x[[piv, c]]
        for r in range(c + 1, n):
            if a[r, c] != 0.0:
                f = a[r, c] / a[c, c]
                a[r, c:] = a[r, c:] - f * a[c, c:]
                x[r] = x[r] - f * x[c]
    for r in range(n - 1, -1, -1):
        for c in range(r + 1, n):
            if a[r, c] != 0.0:
                x[r] = x[r] - a[r, c] * x[c]
        x[r] = x[r] / a[r, r]
    return x


def solve_dense(vals, flags, dts, so):
    """p [S * N][D] float64 as PolyTraj::p(), or None (W < 2: the reference returns false)."""
    vals = np.asarray(vals, dtype=np.float64)
    W, D = vals.shape[1], vals.shape[2]
    if W < 2:
        return None
    N, S = 2 * (so + 1), W - 1
    A, Q, table, nf = _system(W, dts, so, flags, np.float64)
    A, Q = np.array(A, dtype=np.float64), np.array(Q, dtype=np.float64)
    M = np.zeros((S * N, W * N // 2))
    for raw, new in table:
        M[raw, new] = 1.0
    AiM = lu_solve(A, M)
    R = AiM.T @ Q @ AiM
    Dall = np.zeros((W * N // 2, D))
    Df = np.array(_fixed_rows(table, nf, vals, N, D, np.float64), dtype=np.float64).reshape(nf, D)
    Dall[:nf] = Df
    if W * N // 2 - nf > 0:
        Dall[nf:] = -lu_solve(R[nf:, nf:], R[nf:, :nf] @ Df)
    d = M @ Dall
    return np.concatenate([lu_solve(A[i * N:(i + 1) * N, i * N:(i + 1) * N], d[i * N:(i + 1) * N]) for i in range(S)])


def _gauss(Amat, B):
    """Exact dense Gaussian elimination: X with Amat X = B (lists of Fraction rows); None if singular."""
    n, m = len(Amat), len(B[0])
    a = [list(Amat[i]) + list(B[i]) for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if a[r][c] != 0), None)
        if piv is None:
            return None
        a[c], a[piv] = a[piv], a[c]
        inv = 1 / a[c][c]
        a[c] = [x * inv for x in a[c]]
        for r in range(n):
            if r != c and a[r][c] != 0:
                f = a[r][c]
                a[r] = [x - f * y for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


def _exact_parts(vals, flags, dts, so):
    """The exact system: per-segment blocks of A and Q, the map segment-end derivative -> waypoint derivative id, the
    fixed mask and values (Fractions)."""
    vals = np.asarray(vals, dtype=np.float64)
    W, D = vals.shape[1], vals.shape[2]
    N, S, h = 2 * (so + 1), W - 1, so + 1
    A, Q, _, _ = _system(W, dts, so, flags, Fraction)
    Ab = [[row[i * N:(i + 1) * N] for row in A[i * N:(i + 1) * N]] for i in range(S)]
    Qb = [[row[i * N:(i + 1) * N] for row in Q[i * N:(i + 1) * N]] for i in range(S)]
    fixed = [[bool(flags[w] & (1 << k)) for k in range(h)] for w in range(W)]
    val = [[[Fraction(float(vals[k][w][i])) for i in range(D)] for k in range(h)] for w in range(W)]
    return W, D, N, S, h, Ab, Qb, fixed, val


def _exact_R(W, N, S, h, Ab, Qb):
    """R over the W * h waypoint derivatives in waypoint order: sum over segments of A_s^-T Q_s A_s^-1."""
    n = W * h
    R = [[Fraction(0)] * n for _ in range(n)]
    eye = [[Fraction(int(i == j)) for j in range(N)] for i in range(N)]
    for s in range(S):
        Ai = _gauss(Ab[s], eye)
        QA = [[sum(Qb[s][i][m] * Ai[m][j] for m in range(N)) for j in range(N)] for i in range(N)]
        Hs = [[sum(Ai[m][i] * QA[m][j] for m in range(N)) for j in range(N)] for i in range(N)]
        ids = [s * h + k for k in range(h)] + [(s + 1) * h + k for k in range(h)]
        for i in range(N):
            for j in range(N):
                R[ids[i]][ids[j]] += Hs[i][j]
    return R


def solve_exact(vals, flags, dts, so, want_cost=False):
    """The exact minimiser as Fractions: p [S * N][D] (and the cost summed over the axes), or None (W < 2, or a singular
    free system)."""
    if np.asarray(vals).shape[1] < 2:
        return None
    W, D, N, S, h, Ab, Qb, fixed, val = _exact_parts(vals, flags, dts, so)
    R = _exact_R(W, N, S, h, Ab, Qb)
    ids = [(w, k) for w in range(W) for k in range(h)]
    fx = [i for i, (w, k) in enumerate(ids) if fixed[w][k]]
    fr = [i for i, (w, k) in enumerate(ids) if not fixed[w][k]]
    x = [[val[w][k][i] for i in range(D)] for (w, k) in ids]
    if fr:
        rhs = [[-sum(R[i][j] * x[j][a] for j in fx) for a in range(D)] for i in fr]
        sol = _gauss([[R[i][j] for j in fr] for i in fr], rhs)
        if sol is None:
            return None
        for n, i in enumerate(fr):
            x[i] = sol[n]
    p = []
    for s in range(S):
        d = [x[s * h + k] for k in range(h)] + [x[(s + 1) * h + k] for k in range(h)]
        p += _gauss(Ab[s], d)
    if not want_cost:
        return p
    return p, exact_cost(x, R)


def exact_cost(x, R):
    """sum over axes of x^T R x for waypoint derivatives x [W * h][D] (Fractions)."""
    n, D = len(x), len(x[0])
    return sum(x[i][a] * R[i][j] * x[j][a] for a in range(D) for i in range(n) for j in range(n) if R[i][j] != 0)


def exact_setup(vals, flags, dts, so):
    """(R, ids, fixed mask per id) of the exact system, for the optimality test."""
    W, D, N, S, h, Ab, Qb, fixed, val = _exact_parts(vals, flags, dts, so)
    R = _exact_R(W, N, S, h, Ab, Qb)
    ids = [(w, k) for w in range(W) for k in range(h)]
    return R, ids, [fixed[w][k] for (w, k) in ids]


def derivs_of(p, dts, so):
    """End derivatives of the segments of exact coefficients p: ([S][h][D] at 0, [S][h][D] at T) as Fractions."""
    N, h = 2 * (so + 1), so + 1
    S, D = len(p) // N, len(p[0])
    d0 = [[[p[s * N + k][a] * FACT[k] for a in range(D)] for k in range(h)] for s in range(S)]
    dT = []
    for s in range(S):
        T = Fraction(float(dts[s]))
        rows = []
        for k in range(h):
            row = []
            for a in range(D):
                v = Fraction(0)
                for n in range(k, N):
                    c = 1
                    for m in range(k):
                        c *= n - m
                    v += p[s * N + n][a] * c * T ** (n - k)
                row.append(v)
            rows.append(row)
        dT.append(rows)
    return d0, dT


def to_float(p):
    return np.array([[float(x) for x in row] for row in p], dtype=np.float64)


def max_err(p, exact):
    """max |p - exact| over all coefficients, the difference rounded once (p float64 [..][D], exact Fractions)."""
    return max(abs(float(Fraction(float(p[r][a])) - exact[r][a])) for r in range(len(exact)) for a in range(len(exact[0])))


def scale_of(exact):
    return max(abs(float(x)) for row in exact for x in row)


def to_primitive_coeffs(p, so):
    """poly_traj.cpp:72-88: p [S * N][D] -> Vec6f per segment and axis, c [S][D][6] with c_j = p_{5-j} * (5-j)!."""
    p = np.asarray(p, dtype=np.float64)
    N = 2 * (so + 1)
    S, D = p.shape[0] // N, p.shape[1]
    c = np.zeros((S, D, 6))
    for s in range(S):
        for k in range(N):
            c[s, :, 5 - k] = p[s * N + k] * np.float64(FACT[k])
    return c


def yaw_solve(yaw, dts):
    """The yaw solve with yaw_control = VEL (traj_solver.h:87-101): solve_dense of the 1-D problem with every position
    fixed: p [S * 2][1]."""
    W = len(yaw)
    vals = np.zeros((3, W, 1))
    vals[0, :, 0] = yaw
    return solve_dense(vals, np.full(W, USE_POS, np.uint8), dts, 0)


class PolySet(tm.Traj):
    """A solved trajectory as traj_model.Traj lays one out (coef [S][D][6], coef_yaw [S][6], taus, T), built from
    coefficients p [S * N][D], the yaw coefficients [S * 2] and dts: evaluate / sample / traj_model.traverse apply."""

    def __init__(self, p, p_yaw, dts, so, dim):
        self.control, self.dim, self.dt = [VEL, ACC, JRK][so], dim, None
        self.status = 0
        c = to_primitive_coeffs(p, so)
        self.coef = [c[s] for s in range(c.shape[0])]
        self.coef_yaw = []
        for s in range(c.shape[0]):
            cy = np.zeros(6)
            cy[4], cy[5] = p_yaw[2 * s + 1] * np.float64(1), p_yaw[2 * s] * np.float64(1)
            self.coef_yaw.append(cy)
        self.dts = np.asarray(dts, dtype=np.float64)
        self.taus = set_time(self.dts)
        self.S = len(self.coef)
        self.T = float(self.taus[-1])
        effort = [np.float64(0.0)] * 5
        for s in range(self.S):  # Trajectory::J, Primitive::J (primitive.h:92-122) with the segment's own duration
            for o in range(1, 5):
                j = np.float64(0.0)
                for i in range(dim):
                    j = j + tm.effort_1d(self.coef[s][i], self.dts[s], o)
                effort[o - 1] = effort[o - 1] + j
            effort[4] = effort[4] + tm.effort_1d(self.coef_yaw[s], self.dts[s], 1)
        self.effort = np.array(effort, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------- inputs
REF_PATH = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 1.0], [5.0, 1.0]])  # test/test_traj_solver.cpp's path, v = 1


def path_vals(pos, end_vel=None, end_acc=None):
    """vals [3][W][D] of a path: interior derivatives zero (they are free), the ends' as given."""
    pos = np.asarray(pos, dtype=np.float64)
    v = np.zeros((3,) + pos.shape)
    v[0] = pos
    if end_vel is not None:
        v[1, 0], v[1, -1] = end_vel
    if end_acc is not None:
        v[2, 0], v[2, -1] = end_acc
    return v


def random_path(rng, W, D, step=(0.4, 2.5)):
    """A path whose consecutive points differ on every axis' maximum by a step in `step` (no coincident waypoints)."""
    pos = np.zeros((W, D))
    pos[0] = np.round(rng.uniform(-2, 2, D), 3)
    for w in range(1, W):
        d = rng.uniform(-1, 1, D)
        d = d / np.max(np.abs(d)) * rng.uniform(*step)
        pos[w] = pos[w - 1] + np.round(d, 3)
    return pos


def cpu_cases():
    """(name, vals, dts) of the CPU accuracy cases: the reference's own test path, random 3-D paths of 3, 6 and 9
    waypoints with non-zero end derivatives, and a path mixing 0.05 s and 4.9 s segments."""
    rng = np.random.default_rng(2024)
    out = [("ref_path", path_vals(REF_PATH), allocate_time(REF_PATH, 1.0))]
    for W in (3, 6, 9):
        pos = random_path(rng, W, 3)
        ev, ea = np.round(rng.uniform(-1, 1, (2, 3)), 2), np.round(rng.uniform(-1, 1, (2, 3)), 2)
        out.append(("rand%d" % W, path_vals(pos, ev, ea), allocate_time(pos, 0.8)))
    pos = random_path(rng, 6, 3)
    out.append(("mixed_dt", path_vals(pos, np.round(rng.uniform(-1, 1, (2, 3)), 2)), np.array([1.1, 0.05, 4.9, 0.05, 4.9])))
    return out


# ------------------------------------------------------------------------- the kernel's own elimination, restated
HHAT = {1: [[1, -1], [-1, 1]],
        2: [[12, 6, -12, 6], [6, 4, -6, 2], [-12, -6, 12, -6], [6, 2, -6, 4]],
        3: [[720, 360, 60, -720, 360, -60], [360, 192, 36, -360, 168, -24], [60, 36, 9, -60, 24, -3],
            [-720, -360, -60, 720, -360, 60], [360, 168, 24, -360, 192, -36], [-60, -24, -3, 60, -36, 9]]}
BINV = {1: [[1.0]], 2: [[3, -1], [-2, 1]], 3: [[10, -4, 0.5], [-15, 7, -1], [6, -3, 0.5]]}


def _falling(n, q):
    """n! / (n - q)!"""
    r = 1
    for m in range(q):
        r *= n - m
    return r


def solve_block(vals, flags, dts, so):
    """solve_kernel<D, SO> (csrc/solve_kernel.hip) for one problem, in float64, one IEEE operation at a time, in the
    kernel's own order: the same Hhat and B^-1 constants, H = Hhat / T^e with powers by repeated multiply, the
    right-hand sides (carry, then the fixed derivatives of w through G, then those of w + 1 through H[0T]), the Schur
    complement G - C_{w-1}^T Z_{w-1}, the LDL^T without pivoting, the two triangular solves with the division by the
    pivots between them, x_w = z_w - Z_w x_{w+1}, the low half d_k / k! and the high half through binv, divided by
    tp[h + j].  Returns p [S * N][D] as PolyTraj::p(), or None where the kernel reports a status: W < 2 (EMPTY), a
    duration that is not finite or <= 0 (BAD_TIME), a pivot that is not finite or <= 0 (SINGULAR).

    This is a TWIN of the kernel, not an independent reference: it shares the kernel's derivation and would share a
    mistake in it.  solve_exact and solve_dense remain the yardstick of both; what the twin adds is that the device's
    so >= 1 coefficients can be held bit for bit (the kernel is built with -ffp-contract=off and divides truly), so a
    slip in the recursion that stays within the dense model's rounding noise cannot pass."""
    f64 = np.float64
    vals = np.asarray(vals, dtype=np.float64)
    W, D = vals.shape[1], vals.shape[2]
    if W < 2:
        return None
    h = so + 1
    N = 2 * h
    hh, bi = HHAT[h], BINV[h]
    zero, one = f64(0.0), f64(1.0)
    fl = [int(flags[w]) & ((1 << h) - 1) for w in range(W)]
    fact = [f64(FACT[a]) for a in range(N)]
    cur = [[f64(vals[a][0][i]) for i in range(D)] for a in range(h)]
    nx = [[zero] * D for _ in range(h)]
    gtt = [[zero] * h for _ in range(h)]
    cp = [[zero] * h for _ in range(h)]
    zp = [[zero] * h for _ in range(h)]
    carry = [[zero] * D for _ in range(h)]
    zr = [[zero] * D for _ in range(h)]
    Zs, zs, Ts = [], [], []
    fc = fl[0]
    with np.errstate(all="ignore"):
        for w in range(W):
            last = w == W - 1
            H00 = [[zero] * h for _ in range(h)]
            H0T = [[zero] * h for _ in range(h)]
            HTT = [[zero] * h for _ in range(h)]
            fn = 0
            if not last:
                nx = [[f64(vals[a][w + 1][i]) for i in range(D)] for a in range(h)]
                fn = fl[w + 1]
                T = f64(dts[w])
                if not (T > 0.0) or not np.isfinite(T):
                    return None
                Ts.append(T)
                tp = [one]
                for m in range(1, N):
                    tp.append(tp[m - 1] * T)
                for a in range(h):
                    for b in range(h):
                        e = tp[2 * h - 1 - a - b]
                        H00[a][b] = f64(hh[a][b]) / e
                        H0T[a][b] = f64(hh[a][h + b]) / e
                        HTT[a][b] = f64(hh[h + a][h + b]) / e
            G = [[gtt[a][c] + H00[a][c] for c in range(h)] for a in range(h)]
            b = [[zero] * D for _ in range(h)]
            for a in range(h):
                for i in range(D):
                    acc = carry[a][i]
                    for j in range(h):
                        if fc >> j & 1:
                            acc = acc - G[a][j] * cur[j][i]
                    for j in range(h):
                        if not last and (fn >> j & 1):
                            acc = acc - H0T[a][j] * nx[j][i]
                    b[a][i] = cur[a][i] if (fc >> a & 1) else acc
            C = [[zero] * h for _ in range(h)]
            for a in range(h):
                for c in range(h):
                    C[a][c] = H0T[a][c] if (not last and not (fc >> a & 1) and not (fn >> c & 1)) else zero
                    if (fc >> a & 1) or (fc >> c & 1):
                        G[a][c] = one if a == c else zero
            if w > 0:
                for a in range(h):
                    for c in range(a + 1):
                        s = G[a][c]
                        for m in range(h):
                            s = s - cp[m][a] * zp[m][c]
                        G[a][c] = s
                        G[c][a] = s
                    for i in range(D):
                        s = b[a][i]
                        for m in range(h):
                            s = s - cp[m][a] * zr[m][i]
                        b[a][i] = s
            L = [[zero] * h for _ in range(h)]
            dd = [zero] * h
            bad = False
            for j in range(h):
                s = G[j][j]
                for m in range(j):
                    s = s - L[j][m] * L[j][m] * dd[m]
                dd[j] = s
                bad = bad or not (s > 0.0) or not np.isfinite(s)
                for i in range(j + 1, h):
                    q = G[i][j]
                    for m in range(j):
                        q = q - L[i][m] * L[j][m] * dd[m]
                    L[i][j] = q / s
            if bad:
                return None
            X = [[C[a][c] for c in range(h)] + [b[a][i] for i in range(D)] for a in range(h)]
            for c in range(h + D):
                for a in range(h):
                    for m in range(a):
                        X[a][c] = X[a][c] - L[a][m] * X[m][c]
                for a in range(h):
                    X[a][c] = X[a][c] / dd[a]
                for a in range(h - 1, -1, -1):
                    for m in range(a + 1, h):
                        X[a][c] = X[a][c] - L[m][a] * X[m][c]
            zp = [[X[a][c] for c in range(h)] for a in range(h)]
            cp = C
            zr = [[X[a][h + i] for i in range(D)] for a in range(h)]
            Zs.append(zp)
            zs.append(zr)
            gtt = HTT
            carry = [[zero] * D for _ in range(h)]
            for a in range(h):
                for i in range(D):
                    acc = zero
                    for j in range(h):
                        if fc >> j & 1:
                            acc = acc - H0T[j][a] * cur[j][i]
                    carry[a][i] = acc
            if not last:
                cur = nx
                fc = fn
        S = W - 1
        xn = [[cur[a][i] if (fc >> a & 1) else zr[a][i] for i in range(D)] for a in range(h)]
        p = np.zeros((S * N, D))
        for w in range(S - 1, -1, -1):
            x = [[zero] * D for _ in range(h)]
            for a in range(h):
                for i in range(D):
                    s = zs[w][a][i]
                    for j in range(h):
                        s = s - Zs[w][a][j] * xn[j][i]
                    x[a][i] = f64(vals[a][w][i]) if (fl[w] >> a & 1) else s
            T = Ts[w]
            tp = [one]
            for m in range(1, N):
                tp.append(tp[m - 1] * T)
            for i in range(D):
                pl = [x[a][i] / fact[a] for a in range(h)]
                pt = [pl[a] * tp[a] for a in range(h)]
                r = []
                for q in range(h):
                    acc = xn[q][i] * tp[q]
                    for m in range(q, h):
                        acc = acc - f64(_falling(m, q)) * pt[m]
                    r.append(acc)
                for a in range(h):
                    p[w * N + a, i] = pl[a]
                for j in range(h):
                    acc = f64(bi[j][0]) * r[0]
                    for q in range(1, h):
                        acc = acc + f64(bi[j][q]) * r[q]
                    p[w * N + h + j, i] = acc / tp[h + j]
            xn = x
    return p


# ------------------------------------------------------------------- inputs of tests/test_gpu_poly_long.py
LONG_K, LONG_WMAX = 200, 33  # three full waves and eight lanes; up to 32 segments
LONG_NWP = [0, 1, 2, 3, 8, 9, 16, 17, 24, 32, 33, 40]  # n_wp[k] cycles through these; 40 is clamped to w_max
LONG_SEED = 300  # + D; chosen on the CPU with solve_block, see tests/test_gpu_poly_long.py
# the problems that go against solve_exact (W <= 24, every duration pattern), per duration mode
LONG_EXACT = {"given": [3, 6, 16, 19, 29, 32], "alloc_arr": [16, 29]}


def long_w(k):
    return min(LONG_NWP[k % len(LONG_NWP)], LONG_WMAX)


def long_pattern(k):
    """The second problem of every W class alternates 0.05 s / 4.9 s, the third grows geometrically from 0.05 s to 5 s."""
    return {1: "alternating", 2: "geometric"}.get(k // len(LONG_NWP), "random")


_LONG = {}


def long_problems(D):
    """wp [4D+2][33][200] state rows, n_wp [200], dts [32][200], v_arr [200]: computed once per D, never changed.
    Derivative rows as test_gpu_solve.problems; durations random in [0.3, 2.0] rounded to 1e-3, and the two patterns of
    long_pattern, whose problems lie along axis 0 with v = 1 so that allocate_time gives (nearly) the same durations."""
    if D in _LONG:
        return _LONG[D]
    K, WM = LONG_K, LONG_WMAX
    rng = np.random.default_rng(LONG_SEED + D)
    wp = np.zeros((4 * D + 2, WM, K))
    for k in range(K):
        wp[:D, :, k] = random_path(rng, WM, D).T
    wp[D:4 * D] = np.round(rng.uniform(-1, 1, (3 * D, WM, K)), 2)
    wp[4 * D] = rng.uniform(-3, 3, (WM, K))
    v_arr = np.round(rng.uniform(0.4, 2.5, K), 3)
    dts = np.round(rng.uniform(0.3, 2.0, (WM - 1, K)), 3)
    for k in range(K):
        S, pat = long_w(k) - 1, long_pattern(k)
        if S < 1 or pat == "random":
            continue
        dts[:S, k] = [(0.05, 4.9)[s % 2] for s in range(S)] if pat == "alternating" else np.geomspace(0.05, 5.0, S) if S > 1 else [0.05]
        v_arr[k] = 1.0
        step = np.zeros((WM - 1, D))
        step[:, 0] = dts[:, k]
        step[:, 1:] = 0.3 * dts[:, k][:, None]
        wp[:D, 1:, k] = (wp[:D, 0, k][None, :] + np.cumsum(step, axis=0)).T
    n_wp = np.array([LONG_NWP[k % len(LONG_NWP)] for k in range(K)], np.int32)
    for a in (wp, n_wp, dts, v_arr):
        a.setflags(write=False)
    _LONG[D] = (wp, n_wp, dts, v_arr)
    return _LONG[D]


def long_vals(wp, k, W, D):
    return np.stack([wp[a * D:(a + 1) * D, :W, k].T for a in range(3)])  # [3][W][D]


def long_durations(D, mode, k):
    wp, _, dts, v_arr = long_problems(D)
    W = long_w(k)
    if mode == "given":
        return dts[:W - 1, k].copy()
    return allocate_time(wp[:D, :W, k].T, v_arr[k])


def long_flag_problems():
    """The flags set of tests/test_gpu_poly_long.py, setWaypoints mode at W = 17, so = 2, D = 3, K = 5: wp [14][17][5],
    flags [17][5], dts [16][5].  Problem 0: interior waypoints fix (pos); 1: (pos, vel); 2: (vel only) between position
    waypoints; 3: (pos) with every fourth (pos, vel), and an end with a free acceleration; 4: no fixed position anywhere,
    durations powers of two -- the free system is a scalar chain whose pivots stay exact, so the last one is an exact
    zero, not a rounding residue."""
    D, W, Kf = 3, 17, 5
    P, V, A = USE_POS, USE_VEL, USE_ACC
    flags = np.zeros((W, Kf), np.uint8)
    flags[:, 0] = [7] + [P] * (W - 2) + [7]
    flags[:, 1] = [7] + [P | V] * (W - 2) + [7]
    flags[:, 2] = [7] + [P if w % 2 else V for w in range(1, W - 1)] + [7]
    flags[:, 3] = [7] + [P | V if w % 4 == 0 else P for w in range(1, W - 1)] + [P | V]
    flags[:, 4] = V | A
    rng = np.random.default_rng(19)
    wp = np.zeros((4 * D + 2, W, Kf))
    for k in range(Kf):
        wp[:D, :, k] = random_path(rng, W, D).T
    wp[D:3 * D] = np.round(rng.uniform(-1, 1, (2 * D, W, Kf)), 2)
    dts = np.round(rng.uniform(0.4, 1.8, (W - 1, Kf)), 3)
    dts[:, 4] = [1.0, 2.0, 0.5, 1.0] * 4
    return wp, flags, dts
