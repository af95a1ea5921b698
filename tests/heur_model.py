"""The model the dynamics-aware heuristic (include/mplx_heur.h) is compared with, and the inputs of its tests.

A float64 restatement of env_base.h:56-211 (cal_heur with heur_ignore_dynamics_ == false) in its two modes, operation for
operation as csrc/mplx_heur_math.h states them; nothing is shared with the engine.

REFERENCE is the reference with its quirks, for the branches that need no Eigen solver: the candidates of the closed-form
quartic (scale_model.quartic, the C library's cbrt) in its order, then t_bar; control flags compared exactly.  One state
at a time, Python floats.

ROBUST is the true minimum over t >= t_bar of the same cost functions for VEL, ACC and JRK states: the stationary points
are ALL the real roots of the stationary polynomial in (t_bar, T_hi], isolated by the chain of its derivatives and
BISECT halvings each; + - * / sqrt abs and comparisons only, so whole numpy arrays of states go through the same IEEE
operations as one lane of the device does.  h = max(default, min C) -- never below the default, bit for bit.

States are columns: rows pos[D] vel[D] acc[D] jrk[D] yaw (t), as the table and the frontiers hold them."""
import math

import numpy as np

import multi_model as MM
import open_model as OM
import prior_model as PM
import scale_model as SM

DEFAULT, REFERENCE, ROBUST = 0, 1, 2
VEL, ACC, JRK, SNP, YAW = 0x01, 0x03, 0x07, 0x0f, 0x10
BISECT = 56
F = np.float64
DBL_MAX = float(np.finfo(np.float64).max)


def _dot(a, b):
    s = a[0] * b[0]
    for i in range(1, len(a)):
        s = s + a[i] * b[i]
    return s


def _linf(s, g, D):
    m = np.zeros(np.shape(s[0]))
    for i in range(D):  # (d > m ? d : m: a NaN difference is passed over, as post_eval does)
        d = np.abs(s[i] - g[i])
        m = np.where(d > m, d, m)
    return m


def default_heur(s, g, w, v_max, D):
    """env_base.h:58-64 for the columns s: dev::post_eval's expression."""
    s = np.asarray(s, dtype=F)
    L = _linf(s, g, D)
    return w * L / v_max if v_max > 0 else w * L


# ---- REFERENCE --------------------------------------------------------------------------------------------------------

def _ref_quartic_min(c1, c2, c3, w, t_bar):
    ts = SM.quartic(w, F(0.0), c3, c2, c1) + [t_bar]
    cost = F(DBL_MAX)
    for t in ts:
        if t < t_bar:
            continue
        c = -c1 / 3 / t / t / t - c2 / 2 / t / t - c3 / t + w * t
        if c < cost:
            cost = c
    return cost


def reference(s, g, control, goal_control, w, v_max, D):
    """cal_heur of ONE state (a sequence of >= 3D floats) and goal; flags compared exactly.  None: a JRK branch."""
    with np.errstate(all="ignore"):
        s, g = [F(x) for x in s], [F(x) for x in g]
        w, v_max = F(w), F(v_max)
        dp = [g[i] - s[i] for i in range(D)]
        v0, v1 = s[D:2 * D], g[D:2 * D]
        if control == JRK and goal_control in (JRK, ACC, VEL):
            return None
        linf = F(0.0)
        for i in range(D):
            d = abs(s[i] - g[i])
            linf = d if d > linf else linf
        if control == ACC and goal_control == ACC:
            vs = [v0[i] + v1[i] for i in range(D)]
            c1 = -36 * _dot(dp, dp)
            c2 = 24 * _dot(vs, dp)
            c3 = -4 * (_dot(v0, v0) + _dot(v0, v1) + _dot(v1, v1))
            return float(_ref_quartic_min(c1, c2, c3, w, linf / v_max))
        if control == ACC and goal_control == VEL:
            c1 = -9 * _dot(dp, dp)
            c2 = 12 * _dot(v0, dp)
            c3 = -3 * _dot(v0, v0)
            return float(_ref_quartic_min(c1, c2, c3, w, linf / v_max))
        sp = [s[i] - g[i] for i in range(D)]
        norm = np.sqrt(_dot(sp, sp))
        if control == VEL and goal_control == VEL:
            return float((w + 1) * norm)
        return float(w * norm / v_max)


# ---- ROBUST -----------------------------------------------------------------------------------------------------------

def _falling(n, k):
    r = 1
    for i in range(k):
        r *= n - i
    return r


def _horner(q, t):
    r = q[-1]
    for k in range(len(q) - 2, -1, -1):
        r = r * t + q[k]
    return r


def chain_roots(p, lo, hi):
    """The break points x[0 .. N) and their root flags of csrc/mplx_heur_math.h::Chain<N, N>: p[k] the coefficient of
    t^k (arrays of one shape), p[N] > 0."""
    N = len(p) - 1
    q0, q1 = p[N - 1] * F(_falling(N - 1, N - 1)), p[N] * F(_falling(N, N - 1))
    r = -q0 / q1
    r = np.where(r > lo, r, lo)
    r = np.where(r < hi, r, hi)
    x, ok = [r], [np.ones(np.shape(r), bool)]
    for M in range(2, N + 1):
        k = N - M
        q = [p[j + k] * F(_falling(j + k, k)) for j in range(M + 1)]
        a = [lo if i == 0 else x[i - 1] for i in range(M)]
        b = [hi if i == M - 1 else x[i] for i in range(M)]
        na = [_horner(q, a[i]) < 0 for i in range(M)]
        ok = [na[i] != (_horner(q, b[i]) < 0) for i in range(M)]
        top = list(b)
        for _ in range(BISECT):
            for i in range(M):
                m = a[i] + (b[i] - a[i]) * 0.5
                same = (_horner(q, m) < 0) == na[i]
                a[i] = np.where(same, m, a[i])
                b[i] = np.where(same, b[i], m)
        x = [np.where(ok[i], b[i], top[i]) for i in range(M)]
    return x, ok


def _cauchy(p):
    m = 0.0 * p[-1]
    for k in range(len(p) - 1):
        r = np.abs(p[k] / p[-1])
        m = np.where(r > m, r, m)
    return 1.0 + m


def _min_cost(p, t_bar, cost):
    hi = _cauchy(p)
    x, ok = chain_roots(p, t_bar, np.where(hi > t_bar, hi, t_bar))
    best = np.where(t_bar > 0, cost(np.where(t_bar > 0, t_bar, 1.0)), np.inf)
    for i in range(len(x)):
        c = cost(x[i])
        best = np.where(ok[i] & (x[i] > 0) & (c < best), c, best)
    return best


def abs_terms(co, w):
    """t -> sum |terms of C(t)| for the coefficients of coefficients(): the unit the error of h is measured in."""
    if co[0] == "vel":
        return lambda t: np.abs(co[1] / t) + np.abs(w * t)
    if co[0] == "acc":
        return lambda t: np.abs(co[1] / 3 / t / t / t) + np.abs(co[2] / 2 / t / t) + np.abs(co[3] / t) + np.abs(w * t)
    c, d, e, f, g = co[1:]
    return lambda t: (np.abs(w * t) + np.abs(c / t) + np.abs(d / 2 / t / t) + np.abs(e / 3 / t / t / t) + np.abs(f / 4 / t / t / t / t) +
                      np.abs(g / 5 / t / t / t / t / t))


def cost_acc(c1, c2, c3, w):
    return lambda t: -c1 / 3 / t / t / t - c2 / 2 / t / t - c3 / t + w * t


def cost_jrk(a, c, d, e, f, g):
    return lambda t: a * t - c / t - d / 2 / t / t - e / 3 / t / t / t - f / 4 / t / t / t / t - g / 5 / t / t / t / t / t


def coefficients(s, g, cs, cg, w, D):
    """(kind, coefficients) of the pair of BASE controls: ("vel", pp), ("acc", c1, c2, c3), ("jrk", c, d, e, f, g), None."""
    dp = [g[i] - s[i] for i in range(D)]
    v0, v1, a0, a1 = s[D:2 * D], g[D:2 * D], s[2 * D:3 * D], g[2 * D:3 * D]
    if cs == VEL and cg == VEL:
        return ("vel", _dot(dp, dp))
    if cs == ACC and cg == ACC:
        vs = [v0[i] + v1[i] for i in range(D)]
        return ("acc", -36 * _dot(dp, dp), 24 * _dot(vs, dp), -4 * (_dot(v0, v0) + _dot(v0, v1) + _dot(v1, v1)))
    if cs == ACC and cg == VEL:
        return ("acc", -9 * _dot(dp, dp), 12 * _dot(v0, dp), -3 * _dot(v0, v0))
    if cs == JRK and cg == JRK:
        da = [a0[i] - a1[i] for i in range(D)]
        vs = [v0[i] + v1[i] for i in range(D)]
        return ("jrk", -9 * _dot(a0, a0) + 6 * _dot(a0, a1) - 9 * _dot(a1, a1),
                -144 * _dot(a0, v0) - 96 * _dot(a0, v1) + 96 * _dot(a1, v0) + 144 * _dot(a1, v1),
                360 * _dot(da, dp) - 576 * _dot(v0, v0) - 1008 * _dot(v0, v1) - 576 * _dot(v1, v1),
                2880 * _dot(dp, vs), -3600 * _dot(dp, dp))
    if cs == JRK and cg == ACC:
        vm = [1600 * v0[i] + 960 * v1[i] for i in range(D)]
        return ("jrk", -8 * _dot(a0, a0), -112 * _dot(a0, v0) - 48 * _dot(a0, v1),
                240 * _dot(a0, dp) - 384 * _dot(v0, v0) - 432 * _dot(v0, v1) - 144 * _dot(v1, v1), _dot(dp, vm), -1600 * _dot(dp, dp))
    if cs == JRK and cg == VEL:
        return ("jrk", -5 * _dot(a0, a0), -40 * _dot(a0, v0), 60 * _dot(a0, dp) - 60 * _dot(v0, v0), 160 * _dot(dp, v0),
                -100 * _dot(dp, dp))
    return None


def robust(states, goal, control, goal_control, w, v_max, D):
    """heur::robust for the state columns [>= 3D][K]: h [K], without the goal-state rule (heur_eval adds it)."""
    with np.errstate(all="ignore"):
        s = np.asarray(states, dtype=F)
        s = s.reshape(s.shape[0], -1)
        g = [F(x) for x in np.asarray(goal, dtype=F)]
        w, v_max = F(w), F(v_max)
        fin = np.zeros(s.shape[1])
        for i in range(3 * D):
            fin = fin + ((s[i] - s[i]) + (g[i] - g[i]))
        fin = fin + ((w - w) + (v_max - v_max))
        L = _linf(s, g, D)
        h0 = w * L / v_max if v_max > 0 else w * L
        t_bar = L / v_max if v_max > 0 else np.zeros(s.shape[1])
        cs, cg = control & 0x0f, (goal_control if goal_control else control) & 0x0f
        co = coefficients(s, g, cs, cg, w, D)
        if co is None:
            return np.where(fin == 0, h0, np.nan)
        if co[0] == "vel":
            pp = co[1]
            ts = np.sqrt(pp) / np.sqrt(w)
            best = np.where(t_bar > 0, pp / np.where(t_bar > 0, t_bar, 1.0) + w * t_bar, np.inf)
            c = pp / ts + w * ts
            best = np.where((ts > t_bar) & (c < best), c, best)
        elif co[0] == "acc":
            _, c1, c2, c3 = co
            zero = np.zeros(s.shape[1])
            best = _min_cost([c1, c2, c3, zero, w + zero], t_bar, cost_acc(c1, c2, c3, w))
        else:
            _, c, d, e, f, gg = co
            zero = np.zeros(s.shape[1])
            best = _min_cost([gg, f, e, d, c, zero, w + zero], t_bar, cost_jrk(w, c, d, e, f, gg))
        h = np.where((best < np.inf) & (best > h0), best, h0)
        return np.where(fin == 0, h, np.nan)


def same_lattice_state(states, goal, control, goal_control, D):
    """env_base.h:47 per column: the hash of the state under `control` equals the goal's under its own flags."""
    s = np.asarray(states, dtype=F)
    s = s.reshape(s.shape[0], -1)
    gh = PM.lattice_hash(D, goal_control if goal_control else control, [float(x) for x in goal])
    out = np.zeros(s.shape[1], bool)
    for k in range(s.shape[1]):
        col = [float(x) for x in s[:, k]]
        if all(math.isfinite(x) for x in col[:4 * D + 1]):
            out[k] = PM.lattice_hash(D, control, col) == gh
    return out


def heur_eval(states, goal, control, goal_control, w, v_max, D, mode=ROBUST):
    """mplx_heur_eval: get_heur (env_base.h:46-53 without a prior) under `mode` for the columns [4D+1 or more][K]."""
    s = np.asarray(states, dtype=F)
    s = s.reshape(s.shape[0], -1)
    if mode == ROBUST:
        h = robust(s, goal, control, goal_control, w, v_max, D)
    elif mode == DEFAULT:
        h = default_heur(s, [F(x) for x in goal], F(w), F(v_max), D)
    else:
        gc = goal_control if goal_control else control
        h = np.array([reference(s[:, k], goal, control, gc, w, v_max, D) for k in range(s.shape[1])], dtype=F)
    same = same_lattice_state(s, goal, control, goal_control, D)
    return np.where(same & (h == h), 0.0, h)


# ---- the open set with the mode on ------------------------------------------------------------------------------------

class HeurOpenModel(OM.OpenModel):
    """OpenModel whose push takes h from ROBUST (mplx_open_set_heur): `control` the search's, goal_control the goal's."""

    def __init__(self, *a, control=ACC, goal_control=0, **k):
        super().__init__(*a, **k)
        self.control, self.goal_control = control, goal_control
        self._batch = {}

    def heur_and_tol(self, node_id, s):
        h, ok = super().heur_and_tol(node_id, s)
        if int(self.table.hash[node_id]) != self.goal_hash:
            h = self._batch.get(int(node_id))
            if h is None:
                h = float(robust(np.asarray(s, dtype=F)[:, None], self.goal, self.control, self.goal_control, self.w, self.v_max, self.dim)[0])
        return h, ok

    def push(self, fr, n_max, eps, sight=0, capacity=None):
        # the rows of a frontier in one array call: the same IEEE operations per row as one call per row, only faster
        n = min(int(fr["count"]), int(n_max)) if capacity is None else min(int(fr["count"]), int(n_max), int(capacity))
        if n > 1:
            h = robust(np.asarray(fr["state"], dtype=F)[:, :n], self.goal, self.control, self.goal_control, self.w, self.v_max, self.dim)
            self._batch = {int(fr["id"][r]): float(h[r]) for r in range(n)}
        try:
            super().push(fr, n_max, eps, sight, capacity)
        finally:
            self._batch = {}


class HeurMultiOpenModel(MM.MultiOpenModel):
    """MultiOpenModel likewise: every query's own goal and goal_control (goal_controls [Q], 0 = the search's)."""

    def __init__(self, *a, control=ACC, goal_controls=None, **k):
        super().__init__(*a, **k)
        self.control, self.goal_controls = control, goal_controls
        self._batch = {}

    def _gc(self, q):
        return self.goal_controls[q] if self.goal_controls is not None else 0

    def heur_and_tol(self, node_id, s):
        h, ok = super().heur_and_tol(node_id, s)  # (sets self.goal / self.goal_hash to the node's query's)
        q = int(self.table.query[node_id])
        if int(self.table.hash[node_id]) != self.goal_hash:
            h = self._batch.get(int(node_id))
            if h is None:
                h = float(robust(np.asarray(s, dtype=F)[:, None], self.goal, self.control, self._gc(q), self.w, self.v_max, self.dim)[0])
        return h, ok

    def push(self, fr, n_max, eps, sight=0, capacity=None):
        # per query, the rows of the frontier in one array call (as HeurOpenModel.push)
        n = min(int(fr["count"]), int(n_max)) if capacity is None else min(int(fr["count"]), int(n_max), int(capacity))
        ids = [int(i) for i in fr["id"][:n]]
        st = np.asarray(fr["state"], dtype=F)
        self._batch = {}
        for q in range(len(self.goals)):
            rows = [r for r in range(n) if 0 <= ids[r] < self.table.n_nodes and int(self.table.query[ids[r]]) == q]
            if len(rows) > 1:
                h = robust(st[:, rows], self.goals[q], self.control, self._gc(q), self.w, self.v_max, self.dim)
                self._batch.update({ids[r]: float(h[j]) for j, r in enumerate(rows)})
        try:
            super().push(fr, n_max, eps, sight, capacity)
        finally:
            self._batch = {}


# ---- the exact-goal scenario of tests/test_gpu_heur_search.py and tests/test_gpu_heur_plan.py ---------------------------
SCENE_DIMS, SCENE_RES, SCENE_W, SCENE_VMAX = [48, 32], 0.5, 1.0, 2.0
SCENE_START, SCENE_GOAL = (7.25, 5.25), (14.25, 6.25)


def scene_cells(gap=False):
    """48 x 32 cells of 0.5 m: one wall across x = 11 m that leaves the top quarter open; gap: two more free cells low down."""
    c = np.zeros((SCENE_DIMS[1], SCENE_DIMS[0]), np.int8)  # [y][x]
    c[0:24, 22] = 100
    if gap:
        c[9:11, 22] = 0
    return c.ravel()


def scene_rows(starts=(SCENE_START,), goals=(SCENE_GOAL,)):
    """starts [10][Q] and goal rows [Q][10] of 2-D ACC states at rest."""
    s = np.zeros((10, len(starts)))
    g = np.zeros((len(goals), 10))
    s[:2] = np.asarray(starts).T
    g[:, :2] = goals
    return s, g


def scene_search(O, engine, heur, cells=None, start=SCENE_START, goal=SCENE_GOAL, eps=1.0, delta=1.0, capacity=1 << 16, on_round=None):
    """OM.search on the scenario with the oracle's lists: ACC, |U| = 9 (u in {-1, 0, 1}), dt = 1, w = 1, v_max = 2, the
    goal a lattice state with tol_pos = tol_vel = 0 (both heuristics are admissible), no ray trace.  heur: None or
    ROBUST.  Returns (table model, open model, the result of OM.search)."""
    s, g = scene_rows([start], [goal])
    return model_search(O, engine, 2, ACC, scene_cells() if cells is None else cells, SCENE_DIMS, SCENE_RES, SCENE_W, SCENE_VMAX,
                        s[:, 0], g[0], heur, eps, delta, capacity, on_round)


def model_search(O, engine, D, control, cells, dims, res, w, v_max, start, goal, heur, eps=1.0, delta=1.0, capacity=1 << 16,
                 on_round=None):
    """OM.search with the oracle's lists: u in {-1, 0, 1}^D, dt = 1, a_max = j_max = 1, an exact goal state."""
    from table_model import TableModel, oracle_provider
    U = engine.workloads.grid_controls([-1.0, 0.0, 1.0], D)
    oenv = O.Env(D, control, U, cells, dims, [0.0] * D, res, dt=1.0, w=w, v_max=v_max, a_max=1.0, j_max=1.0)
    table = TableModel(4 * D + 2)
    cls, kw = (HeurOpenModel, dict(control=control, goal_control=0)) if heur == ROBUST else (OM.OpenModel, {})
    opn = cls(table, D, goal, O.lattice_hash(D, control, goal), w, v_max, tol_pos=0.0, tol_vel=0.0, tol_acc=0.0 if control == JRK else -1.0, **kw)
    out = OM.search(table, opn, oracle_provider(O, oenv), start, O.lattice_hash(D, control, start), eps, delta, capacity,
                    sight=0, on_round=on_round)
    return table, opn, out


# the 3-D JRK scenario: 16^3 cells of 0.5 m, a slab with a hole between the start and the goal, both at rest
SCENE3_DIMS, SCENE3_START, SCENE3_GOAL = [16, 16, 16], (2.25, 3.25, 3.25), (5.25, 3.25, 3.25)


def scene3_cells():
    c = np.zeros((16, 16, 16), np.int8)  # [z][y][x]
    c[:, :, 7] = 100
    c[5:9, 5:9, 7] = 0
    return c.ravel()


def scene3_search(O, engine, heur, **kw):
    s, g = np.zeros(14), np.zeros(14)
    s[:3], g[:3] = SCENE3_START, SCENE3_GOAL
    return model_search(O, engine, 3, JRK, scene3_cells(), SCENE3_DIMS, SCENE_RES, SCENE_W, SCENE_VMAX, s, g, heur, **kw)


# ---- the exact minimum, in extended precision --------------------------------------------------------------------------

def exact_min(kind, co, w, t_bar):
    """(h*, n_pos, where, scale) of ONE state from float coefficients taken as exact: the minimum of C over t >= t_bar
    (None when there is no candidate), the number of positive stationary points, "bar" / "interior" for where the
    minimum lies, and sum |terms of C| at the minimiser.  mpmath at 60 digits."""
    import mpmath as mp
    mp.mp.dps = 60
    w, t_bar = mp.mpf(float(w)), mp.mpf(float(t_bar))
    co = [mp.mpf(float(x)) for x in co]
    if kind == "vel":
        poly = [w, 0, -co[0]]  # w t^2 - pp
        terms = lambda t: [co[0] / t, w * t]
    elif kind == "acc":
        c1, c2, c3 = co
        poly = [w, 0, c3, c2, c1]
        terms = lambda t: [-c1 / 3 / t ** 3, -c2 / 2 / t ** 2, -c3 / t, w * t]
    else:
        c, d, e, f, g = co
        poly = [w, 0, c, d, e, f, g]
        terms = lambda t: [w * t, -c / t, -d / 2 / t ** 2, -e / 3 / t ** 3, -f / 4 / t ** 4, -g / 5 / t ** 5]
    while len(poly) > 1 and poly[-1] == 0:  # roots at 0 are no stationary points
        poly = poly[:-1]
    roots = mp.polyroots(poly, maxsteps=500, extraprec=400) if len(poly) > 1 else []
    tol = mp.mpf(10) ** -40
    pos = sorted(mp.re(r) for r in roots if abs(mp.im(r)) <= tol * (1 + abs(r)) and mp.re(r) > 0)
    cands = ([(t_bar, "bar")] if t_bar > 0 else []) + [(t, "interior") for t in pos if t > t_bar]
    if not cands:
        return None, len(pos), None, None
    vals = [(sum(terms(t)), wh, t) for t, wh in cands]
    v, wh, t = min(vals, key=lambda z: z[0])
    return v, len(pos), wh, sum(abs(x) for x in terms(t))


def lattice_states(rng, K, D, kind, speed=3.0, span=6.0, zero_dp=0.0):
    """K random 0.25-lattice state columns [4D+2][K]: positions in +-span, velocities (and accelerations for JRK) up to
    `speed`; a share zero_dp of them sit on the goal's position (the goal is the origin state of goal_row())."""
    s = np.zeros((4 * D + 2, K))
    q = lambda lim: rng.integers(-int(lim * 4), int(lim * 4) + 1, (D, K)).astype(F) / 4.0
    s[:D] = q(span)
    if kind != VEL:
        s[D:2 * D] = q(speed)
    if kind == JRK:
        s[2 * D:3 * D] = q(speed)
    s[:D, rng.random(K) < zero_dp] = 0.0
    return s


# ---- the sweeps of tests/test_heur_model.py and profiles/micro/heur_dyn_error.py ---------------------------------------
BRANCHES = [(VEL, VEL), (ACC, ACC), (ACC, VEL), (JRK, JRK), (JRK, ACC), (JRK, VEL)]
SWEEP_SETTINGS = [(1.0, 2.0), (0.5, 1.0), (1.0, 0.5), (0.25, 3.0)]  # (w, v_max): w <= 1 and a slow robot put minima at t_bar


def sweep_goal(D, cg):
    g = np.zeros(4 * D + 2)
    if cg >= ACC:
        g[D:2 * D] = [0.5, -0.25, 0.25][:D]
    if cg >= JRK:
        g[2 * D:3 * D] = [-0.25, 0.5, 0.0][:D]
    return g


def sweep_states(branch, D, n, seed, three_share=0.0):
    """n lattice columns of branch (cs, cg) in D dimensions, a twentieth of them on the goal's position.  three_share:
    that share of the columns is drawn from those whose stationary polynomial has three positive real roots by
    numpy.roots under w = 1 (a cheap float pre-selection; the tests count with the exact roots)."""
    cs, cg = branch
    rng = np.random.default_rng(seed)
    goal = sweep_goal(D, cg)
    s = lattice_states(rng, n, D, cs, zero_dp=0.05)
    want = int(n * three_share)
    if want and cs != VEL:
        got, tries = [], 0
        while len(got) < want and tries < 40:
            tries += 1
            c = lattice_states(rng, 2000, D, cs)
            co = coefficients(c, [F(x) for x in goal], cs, cg, F(1.0), D)
            for k in range(c.shape[1]):
                p = [1.0, 0.0] + ([co[3][k], co[2][k], co[1][k]] if co[0] == "acc" else [co[1][k], co[2][k], co[3][k], co[4][k], co[5][k]])
                r = np.roots(p)
                if np.sum((np.abs(r.imag) < 1e-9) & (r.real > 0)) >= 3:
                    got.append(c[:, k])
                    if len(got) == want:
                        break
        if got:
            s[:, :len(got)] = np.array(got).T
    return s, goal


def sweep_units(branch, D, s, goal, w, v_max):
    """Per column: (|h - h*| in units of 2^-52 sum |terms of C at the minimiser|, positive stationary points, where the
    minimum lies ("bar", "interior", "default" where the default heuristic is the larger, None without a candidate), h,
    h* as a float, that sum as a float)."""
    import mpmath as mp
    cs, cg = branch
    h = robust(s, goal, cs, cg, w, v_max, D)
    d = default_heur(s, [F(x) for x in goal], F(w), F(v_max), D)
    t_bar = _linf(s, [F(x) for x in goal], D) / F(v_max) if v_max > 0 else np.zeros(s.shape[1])
    out = []
    for k in range(s.shape[1]):
        co = coefficients([F(x) for x in s[:, k]], [F(x) for x in goal], cs, cg, F(w), D)
        hs, npos, where, scale = exact_min(co[0], co[1:], w, t_bar[k])
        if hs is None:
            out.append((0.0 if h[k] == d[k] else np.inf, npos, None, float(h[k]), float(d[k]), 0.0))
            continue
        if not hs > mp.mpf(float(d[k])):
            hs, where = mp.mpf(float(d[k])), "default"
        u = abs(mp.mpf(float(h[k])) - hs) / (mp.mpf(2) ** -52 * scale) if scale > 0 else mp.mpf(0)
        out.append((float(u), npos, where, float(h[k]), float(hs), float(scale)))
    return out
