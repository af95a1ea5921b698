"""The model the trajectory calls (include/mplx_traj.h) are compared with, and the inputs of their tests.

A numpy restatement of Trajectory<Dim> (trajectory.h: the chain of forward primitives, taus by sequential addition,
evaluate in both forms, sample, J, Jyaw) and of env_map::traverse_trajectory (env_map.h:229-255) with the full
expressions of primitive.h -- c0 included, as an array of zeros -- so that it does not share the kernel's shortened
forms.  tests/test_traj.py pins it bit for bit to tests/golden/traj_golden.npz, which the reference's own classes
wrote (tests/golden/make_traj_golden.py); tests/test_gpu_traj.py compares the device with it.

fixture_cases(): the inputs of the fixture; gpu_case(): the larger sets of the GPU tests."""
import numpy as np

CONTROLS = [0x01, 0x03, 0x07, 0x0F, 0x11, 0x13, 0x17, 0x1F]
EMPTY, BAD_ACTION, BAD = 1, 2, 4
COMMAND, WAYPOINT = 0, 1
HORIZON = 5
PI = float(np.pi)

MAP2 = ([40, 33], [-1.5, 0.7], 0.25)
MAP3 = ([24, 21, 19], [-1.0, 0.5, -0.3], 0.25)


def order_of(control):
    return {1: 1, 3: 2, 7: 3, 15: 4}[control & 0x0F]


def pw(t, n):
    r = np.ones_like(t)
    for _ in range(n):
        r = r * t
    return r


def normalize_angle(a):
    a = np.array(a, dtype=np.float64, copy=True)
    while (a > PI).any():
        a = np.where(a > PI, a - 2.0 * PI, a)
    while (a < -PI).any():
        a = np.where(a < -PI, a + 2.0 * PI, a)
    return a


# primitive.h:128-145 on coefficient arrays c[0..5]
def poly_p(c, t):
    return c[0] / 120 * pw(t, 5) + c[1] / 24 * pw(t, 4) + c[2] / 6 * pw(t, 3) + c[3] / 2 * t * t + c[4] * t + c[5]


def poly_v(c, t):
    return c[0] / 24 * pw(t, 4) + c[1] / 6 * pw(t, 3) + c[2] / 2 * t * t + c[3] * t + c[4]


def poly_a(c, t):
    return c[0] / 6 * pw(t, 3) + c[1] / 2 * t * t + c[2] * t + c[3]


def poly_j(c, t):
    return c[0] / 2 * t * t + c[1] * t + c[2]


def effort_1d(c, t, order):
    """primitive.h:92-122."""
    c0, c1, c2, c3, c4 = c[0], c[1], c[2], c[3], c[4]
    if order == 1:
        return (c0 * c0 / 5184 * pw(t, 9) + c0 * c1 / 576 * pw(t, 8) + (c1 * c1 / 252 + c0 * c2 / 168) * pw(t, 7) +
                (c0 * c3 / 72 + c1 * c2 / 36) * pw(t, 6) + (c2 * c2 / 20 + c0 * c4 / 60 + c1 * c3 / 15) * pw(t, 5) +
                (c2 * c3 / 4 + c1 * c4 / 12) * pw(t, 4) + (c3 * c3 / 3 + c2 * c4 / 3) * pw(t, 3) + c3 * c4 * t * t + c4 * c4 * t)
    if order == 2:
        return (c0 * c0 / 252 * pw(t, 7) + c0 * c1 / 36 * pw(t, 6) + (c1 * c1 / 20 + c0 * c2 / 15) * pw(t, 5) +
                (c0 * c3 / 12 + c1 * c2 / 4) * pw(t, 4) + (c2 * c2 / 3 + c1 * c3 / 3) * pw(t, 3) + c2 * c3 * t * t + c3 * c3 * t)
    if order == 3:
        return (c0 * c0 / 20 * pw(t, 5) + c0 * c1 / 4 * pw(t, 4) + (c1 * c1 + c0 * c2) / 3 * pw(t, 3) + c1 * c2 * t * t +
                c2 * c2 * t)
    return c0 * c0 / 3 * pw(t, 3) + c0 * c1 * t * t + c1 * c1 * t


def coefficients(control, state, u, dim):
    """Per axis the Vec6f of primitive.h:34-50, [D][6], and the yaw primitive's [6]."""
    K = order_of(control)
    c = np.zeros((dim, 6))
    for i in range(dim):
        p, v, a, j = (state[r * dim + i] for r in range(4))
        c[i] = {1: [0, 0, 0, 0, u[i], p], 2: [0, 0, 0, u[i], v, p], 3: [0, 0, u[i], a, v, p], 4: [0, u[i], j, a, v, p]}[K]
    cy = np.zeros(6)
    if control & 0x10:
        cy[4], cy[5] = u[dim], state[4 * dim]
    return c, cy


class Traj:
    """One trajectory: segments, taus, chain states, efforts."""

    def __init__(self, control, dim, dt, U, start, actions):
        self.control, self.dim, self.dt = control, dim, float(dt)
        self.status = 0
        s = np.array(start, dtype=np.float64)
        self.states = [s.copy()]
        self.coef, self.coef_yaw, self.taus = [], [], [np.float64(0.0)]
        one = np.float64(dt)
        effort = [np.float64(0.0)] * 5
        for a in actions:
            a = int(a)
            if a == -1:
                break
            if a < -1 or a >= len(U):
                self.status |= BAD_ACTION
                break
            c, cy = coefficients(control, s, U[a], dim)
            self.coef.append(c)
            self.coef_yaw.append(cy)
            self.taus.append(one + self.taus[-1])  # trajectory.h:54
            for o in range(1, 5):
                j = np.float64(0.0)
                for i in range(dim):
                    j = j + effort_1d(c[i], one, o)
                effort[o - 1] = effort[o - 1] + j
            effort[4] = effort[4] + effort_1d(cy, one, 1)
            n = np.zeros_like(s)
            for i in range(dim):
                n[i], n[dim + i] = poly_p(c[i], one), poly_v(c[i], one)
                n[2 * dim + i], n[3 * dim + i] = poly_a(c[i], one), poly_j(c[i], one)
            n[4 * dim] = normalize_angle(poly_p(cy, one)) if control & 0x10 else 0.0
            n[4 * dim + 1] = s[4 * dim + 1] + one
            s = n
            self.states.append(s.copy())
        self.S = len(self.coef)
        if self.S == 0:
            self.status |= EMPTY
        self.T = float(self.taus[-1])
        self.effort = np.array(effort, dtype=np.float64)
        self.taus = np.array(self.taus, dtype=np.float64)

    def _segment(self, tau, command):
        lo, hi = self.taus[:-1][:, None], self.taus[1:][:, None]
        if command:
            m = (tau[None, :] >= lo) & (tau[None, :] <= hi)
        else:
            m = (tau[None, :] >= lo) & (tau[None, :] < hi)
            m[-1, :] = True
        assert m.any(0).all()
        return m.argmax(0)

    def evaluate(self, times, form):
        """Rows [4D+3][Q] (COMMAND) or [4D+1][Q] (WAYPOINT) at `times`; a non-finite time gives NaN rows."""
        D = self.dim
        times = np.asarray(times, dtype=np.float64)
        ok = np.isfinite(times)
        tau = np.where(ok, times, 0.0)
        tau = np.where(tau < 0, 0.0, tau)
        tau = np.where(tau > self.T, self.T, tau)
        seg = self._segment(tau, form == COMMAND)
        t = tau - self.taus[seg]
        coef = np.stack(self.coef)[seg]          # [Q][D][6]
        cy = np.stack(self.coef_yaw)[seg].T      # [6][Q]
        rows = np.zeros((4 * D + (3 if form == COMMAND else 1), len(times)))
        lam, lam_dot = np.float64(1.0), np.float64(0.0)
        with np.errstate(all="ignore"):
            for i in range(D):
                c = coef[:, i, :].T
                p, v, a, j = poly_p(c, t), poly_v(c, t), poly_a(c, t), poly_j(c, t)
                if form == COMMAND:  # trajectory.h:118-124
                    vel = v / lam
                    acc = a / lam / lam - vel * lam_dot / lam / lam / lam
                    jrk = j / lam / lam - 3 / pw(lam, 3) * acc * acc * lam_dot + 3 / pw(lam, 4) * vel * lam_dot * lam_dot
                else:
                    vel, acc, jrk = v, a, j
                rows[i], rows[D + i], rows[2 * D + i], rows[3 * D + i] = p, vel, acc, jrk
            rows[4 * D] = normalize_angle(poly_p(cy, t))
            if form == COMMAND:
                rows[4 * D + 1] = normalize_angle(poly_v(cy, t))
                rows[4 * D + 2] = times
        rows[:, ~ok] = np.nan
        return rows

    def sample(self, N, form=COMMAND):
        step = np.float64(self.T) / np.float64(N)  # trajectory.h:233
        return self.evaluate(np.arange(N + 1).astype(np.float64) * step, form)


def c_round(x):
    """std::round: half away from zero."""
    t = np.trunc(x)
    return np.where(np.abs(x - t) >= 0.5, t + np.sign(x), t)  # (x - trunc(x) is exact)


def cell_index(pos, md, org, res):
    """floatToInt + getIndex in wrapping int32 arithmetic for positions [D][Q]: (idx int32 [Q], outside bool [Q])."""
    D = len(md)
    with np.errstate(all="ignore"):
        c = c_round((pos - np.asarray(org, dtype=np.float64)[:, None]) / res - 0.5)
    c = np.where(np.isnan(c), -2147483648.0, np.clip(c, -2147483648.0, 2147483647.0)).astype(np.int64)
    outside = np.zeros(pos.shape[1], bool)
    idx = np.zeros(pos.shape[1], np.int64)
    mul = 1
    for i in range(D):
        outside |= (c[i] < 0) | (c[i] >= md[i])
        idx = idx + c[i] * mul
        mul *= md[i]
    idx = ((idx + 2 ** 31) % 2 ** 32) - 2 ** 31
    return idx.astype(np.int32), outside


def traverse(tr, grid, pot, md, org, res, v_max, pot_w, grad_w):
    """env_map.h:229-255 for one Traj: dict(status, cost, n_samples, n_cells, stop_sample)."""
    if tr.S == 0:
        return {"status": tr.status, "cost": 0.0, "n_samples": 0, "n_cells": 0, "stop_sample": -1}
    with np.errstate(all="ignore"):
        cn = np.ceil(np.float64(v_max) * np.float64(tr.T) / np.float64(res))
    if not cn < 2147483648.0:
        return {"status": tr.status | BAD, "cost": np.nan, "n_samples": 0, "n_cells": 0, "stop_sample": -1}
    n = int(cn)
    rows = tr.sample(n)
    D = tr.dim
    idx, outside = cell_index(rows[:D], md, org, res)
    vel = rows[D:2 * D]
    q = vel[0] * vel[0]
    for i in range(1, D):
        q = q + vel[i] * vel[i]
    norm = np.sqrt(q)
    cost, prev, n_cells = np.float64(0.0), -1, 0
    for i in range(n + 1):
        k = int(idx[i])
        if k == prev:
            continue
        prev = k
        n_cells += 1
        if outside[i]:
            return {"status": tr.status, "cost": np.inf, "n_samples": n + 1, "n_cells": n_cells, "stop_sample": i}
        if pot is not None:
            pv = int(pot[k])
            if 0 < pv < 100:
                cost = cost + (np.float64(pot_w) * np.float64(pv) + np.float64(grad_w) * norm[i])
            elif pv >= 100:
                return {"status": tr.status, "cost": np.inf, "n_samples": n + 1, "n_cells": n_cells, "stop_sample": i}
        elif int(grid[k]) == 100:
            return {"status": tr.status, "cost": np.inf, "n_samples": n + 1, "n_cells": n_cells, "stop_sample": i}
    return {"status": tr.status, "cost": float(cost), "n_samples": n + 1, "n_cells": n_cells, "stop_sample": -1}


def traverse_set(trajs, *args):
    rs = [traverse(t, *args) for t in trajs]
    return {"status": np.array([r["status"] for r in rs], np.uint8), "cost": np.array([r["cost"] for r in rs], np.float64),
            "n_samples": np.array([r["n_samples"] for r in rs], np.int32), "n_cells": np.array([r["n_cells"] for r in rs], np.int32),
            "stop_sample": np.array([r["stop_sample"] for r in rs], np.int32)}


# ---------------------------------------------------------------------------------------------------------- inputs
def control_table(control, dim, rng=None):
    """3^D spatial combinations of {-u, 0, u} (u = 1 for VEL and ACC, larger for JRK and SNP so that the paths bend
    within a few segments), x 3 yaw rates with the yaw bit."""
    u = {1: 1.0, 2: 1.0, 3: 2.0, 4: 4.0}[order_of(control)]
    axes = np.array([-u, 0.0, u])
    grids = np.meshgrid(*([axes] * dim), indexing="ij")
    U = np.stack([g.ravel() for g in grids], axis=1)
    if control & 0x10:
        U = np.concatenate([np.concatenate([U, np.full((len(U), 1), y)], axis=1) for y in (-0.9, 0.0, 0.9)])
    return np.ascontiguousarray(U)


def make_map(md, seed):
    """Occupancy cells (mostly free, 6 % occupied, a few unknown and odd values) and a potential map with values -1 .. 100."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(md))
    grid = np.zeros(n, np.int8)
    r = rng.random(n)
    grid[r < 0.06] = 100
    grid[(r >= 0.06) & (r < 0.08)] = -1
    grid[(r >= 0.08) & (r < 0.09)] = 37
    grid[(r >= 0.09) & (r < 0.095)] = 101
    pot = np.zeros(n, np.int8)
    r = rng.random(n)
    band = (r >= 0.03) & (r < 0.45)
    pot[band] = rng.integers(1, 100, size=n)[band].astype(np.int8)
    pot[r < 0.03] = 100
    pot[r >= 0.97] = -1
    return grid, pot


def starts_and_actions(control, dim, md, org, res, K, nU, seed, lengths=None, border=0.35):
    """K start states (4D+2 rows; a share `border` of them within a cell or two of the map's border) and actions
    [HORIZON][K] with lengths 0 .. HORIZON (k mod 6 unless given)."""
    rng = np.random.default_rng(seed)
    F = 4 * dim + 2
    ext = np.asarray(md) * res
    starts = np.zeros((F, K))
    near = rng.random(K) < border
    for i in range(dim):
        inner = org[i] + ext[i] * (0.15 + 0.7 * rng.random(K))
        side = rng.random(K) < 0.5
        edge = np.where(side, org[i] + res * (0.2 + 1.5 * rng.random(K)), org[i] + ext[i] - res * (0.2 + 1.5 * rng.random(K)))
        starts[i] = np.where(near & (rng.random(K) < 0.7), edge, inner)
    K_ord = order_of(control)
    if K_ord >= 2:
        starts[dim:2 * dim] = np.round(rng.uniform(-1, 1, (dim, K)), 1)
    if K_ord >= 3:
        starts[2 * dim:3 * dim] = np.round(rng.uniform(-1, 1, (dim, K)), 1)
    if K_ord >= 4:
        starts[3 * dim:4 * dim] = np.round(rng.uniform(-1, 1, (dim, K)), 1)
    if control & 0x10:
        starts[4 * dim] = rng.uniform(-3.0, 3.0, K)
    starts[4 * dim + 1] = np.round(rng.uniform(0, 3, K), 2)
    actions = rng.integers(0, nU, size=(HORIZON, K)).astype(np.int32)
    if lengths is None:
        lengths = np.arange(K) % (HORIZON + 1)
    for h in range(HORIZON):
        actions[h, lengths <= h] = -1
    return starts, actions


def query_times(T, taus, rng):
    """Caller times for one trajectory: below 0, above T, 0, T, every taus entry, and a few inside."""
    q = [-0.37, -1e-300, 0.0, T, T + 0.25, 1e9] + [float(x) for x in taus[1:-1]]
    q += [float(x) for x in rng.uniform(0, max(T, 0.5), 4)]
    return q


V_MAX = 2.0
POT_W = 0.1
UNIFORM_N = 5
QUERIES = 12  # per trajectory in the fixture (padded with interior times / cut)


def fixture_cases():
    """The inputs of the fixture, dicts: 8 controls x 2 dims x dt in (0.7, 1.0) with six trajectories each of 0 .. 5
    segments on the two maps, then the hand cases."""
    out = []
    for dim, geo in ((2, MAP2), (3, MAP3)):
        md, org, res = geo
        grid, pot = make_map(md, 40 + dim)
        for control in CONTROLS:
            for dt in (0.7, 1.0):
                U = control_table(control, dim)
                seed = 1000 * dim + 10 * control + int(dt * 10)
                starts, actions = starts_and_actions(control, dim, md, org, res, 6, len(U), seed)
                out.append({"name": "d%d_c%02x_dt%02d" % (dim, control, int(dt * 10)), "control": control, "dim": dim, "dt": dt,
                            "U": U, "starts": starts, "actions": actions, "geo": geo, "grid": grid, "pot": pot, "v_max": V_MAX})
    md, org, res, U, start, actions, dt, v_max = alias_case()
    free = np.zeros(64, np.int8)
    out.append({"name": "hand_alias", "control": 0x01, "dim": 2, "dt": dt, "U": U, "starts": start.reshape(-1, 1),
                "actions": actions, "geo": (md, org, res), "grid": free, "pot": free.copy(), "v_max": v_max})
    U, start, actions, dt = boundary_case()
    geo = ([8, 8], [-4.0, -4.0], 1.0)
    out.append({"name": "hand_boundary", "control": 0x03, "dim": 2, "dt": dt, "U": U, "starts": start.reshape(-1, 1),
                "actions": actions, "geo": geo, "grid": free, "pot": free.copy(), "v_max": V_MAX})
    out.append({"name": "hand_4x07", "control": 0x01, "dim": 2, "dt": 0.7, "U": np.array([[1.0, 0.0], [0.0, 0.5]]),
                "starts": start.reshape(-1, 1), "actions": np.array([[0], [1], [0], [1]], np.int32), "geo": geo, "grid": free,
                "pot": free.copy(), "v_max": V_MAX})
    return out


def case_trajs(case):
    return build_set(case["control"], case["dim"], case["dt"], case["U"], case["starts"], case["actions"])


def fixture_queries(case, trajs):
    rng = np.random.default_rng(7)
    Q = np.zeros((len(trajs), QUERIES))
    for k, tr in enumerate(trajs):
        q = query_times(tr.T, tr.taus, rng)
        q = (q + [float(x) for x in rng.uniform(0, max(tr.T, 0.5), QUERIES)])[:QUERIES]
        Q[k] = q
    return Q


MODES = [("occ", False, 0.0), ("pot_g0", True, 0.0), ("pot_g25", True, 0.25)]


def build_set(control, dim, dt, U, starts, actions):
    return [Traj(control, dim, dt, U, starts[:, k if starts.shape[1] > 1 else 0], actions[:, k]) for k in range(actions.shape[1])]


# ---- hand cases (ISSUE: the index alias, the boundary pair, 4 x 0.7, times below 0 and above T)
def alias_case():
    """8 x 8 map, res 1, origin 0, VEL control: from the centre of cell (0, 3) one segment with u = (8, -1), dt = 1 and
    v_max = 1 give n = 1: sample 0 in cell (0, 3) (index 24), sample 1 in cell (8, 2) -- outside, index 8 + 8 * 2 = 24,
    skipped.  The reference returns 0."""
    md, org, res = [8, 8], [0.0, 0.0], 1.0
    U = np.array([[8.0, -1.0], [1.0, 0.0]])
    start = np.zeros(10)
    start[0], start[1] = 0.5, 3.5
    return md, org, res, U, start, np.array([[0]], np.int32), 1.0, 1.0  # ..., dt, v_max


def boundary_case():
    """ACC controls 0.5 then -0.5 (1D motion along x in 2D), dt = 1: at t = 1.0 the Command has acc 0.5, the Waypoint -0.5."""
    U = np.array([[0.5, 0.0], [-0.5, 0.0]])
    return U, np.zeros(10), np.array([[0], [1]], np.int32), 1.0


# ---- the sets of the GPU tests
GPU_K = 193


def gpu_case(control, dim):
    md, org, res = MAP2 if dim == 2 else MAP3
    grid, pot = make_map(md, 40 + dim)
    U = control_table(control, dim)
    starts, actions = starts_and_actions(control, dim, md, org, res, GPU_K, len(U), 77 + control + dim)
    return U, starts, actions, (md, org, res), grid, pot
