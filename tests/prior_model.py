"""A plain sequential restatement of include/mplx_prior.h: env_map::set_prior_trajectory (reference env_map.h:189-226,
with traverse_trajectory :229-255 and Trajectory / Primitive1D of mpl_basis) and env_base::get_heur with a prior
(env_base.h:46-53).  Test infrastructure: Python floats (IEEE doubles, no contraction) and loops, nothing shared with the
engine.  PriorOpenModel / PriorMultiOpenModel put the heuristic rule on tests/open_model.py and tests/multi_model.py.
"""
import math

import numpy as np

import multi_model as MM
import open_model as OM

EMPTY, BAD_ACTION, BAD = 1, 2, 4  # MPLX_TRAJ_*
INF = math.inf


def _order(control):
    return 4 if control & 8 else 3 if control & 4 else 2 if control & 2 else 1


def _round_away(x):
    """std::round: half away from zero."""
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1
    return int(-r if x < 0 else r)


def _wrap32(v):
    v &= 0xffffffff
    return v - (1 << 32) if v >= (1 << 31) else v


def lattice_hash(dim, control, row):
    """waypoint.h:93-125: boost::hash_combine (classic form) over the quantised rows the control flag uses."""
    M = (1 << 64) - 1
    h = 0

    def fold(h, i):
        return h ^ (((i & M) + 0x9e3779b9 + ((h << 6) & M) + (h >> 2)) & M)
    for i in range(dim):
        if control & 1:
            h = fold(h, _round_away(row[0 * dim + i] / 0.01))
        if control & 2:
            h = fold(h, _round_away(row[1 * dim + i] / 0.1))
        if control & 4:
            h = fold(h, _round_away(row[2 * dim + i] / 0.1))
        if control & 8:
            h = fold(h, _round_away(row[3 * dim + i] / 0.1))
    if control & 16:
        h = fold(h, _round_away(row[4 * dim] / 0.1))
    return h


def _power(x, n):
    r = 1.0
    for _ in range(n):
        r *= x
    return r


def _p(c, t):  # Primitive1D::p, primitive.h:128-131
    return c[0] / 120 * _power(t, 5) + c[1] / 24 * _power(t, 4) + c[2] / 6 * _power(t, 3) + c[3] / 2 * t * t + c[4] * t + c[5]


def _v(c, t):  # primitive.h:133-137
    return c[0] / 24 * _power(t, 4) + c[1] / 6 * _power(t, 3) + c[2] / 2 * t * t + c[3] * t + c[4]


def _a(c, t):  # primitive.h:140-142
    return c[0] / 6 * _power(t, 3) + c[1] / 2 * t * t + c[2] * t + c[3]


def _j(c, t):  # primitive.h:145
    return c[0] / 2 * t * t + c[1] * t + c[2]


def _wrap_pi(a):
    while a > math.pi:
        a -= 2.0 * math.pi
    while a < -math.pi:
        a += 2.0 * math.pi
    return a


def _coeffs(dim, K, s, u):
    """Primitive1D coefficient vectors of a forward primitive from state s with control u (primitive.h:34-50)."""
    out = []
    for i in range(dim):
        c = [0.0] * 6
        c[5] = s[i]
        if K == 1:
            c[4] = u[i]
        elif K == 2:
            c[4], c[3] = s[dim + i], u[i]
        elif K == 3:
            c[4], c[3], c[2] = s[dim + i], s[2 * dim + i], u[i]
        else:
            c[4], c[3], c[2], c[1] = s[dim + i], s[2 * dim + i], s[3 * dim + i], u[i]
        out.append(c)
    return out


def _waypoint(dim, control, cs, s, u, t):
    """Primitive::evaluate(t) -> Waypoint rows (primitive.h:321-331); the yaw primitive only with the yaw bit."""
    row = [0.0] * (4 * dim + 2)
    for i in range(dim):
        row[i], row[dim + i], row[2 * dim + i], row[3 * dim + i] = _p(cs[i], t), _v(cs[i], t), _a(cs[i], t), _j(cs[i], t)
    if control & 16:
        cy = [0.0, 0.0, 0.0, 0.0, u[dim], s[4 * dim]]
        row[4 * dim] = _wrap_pi(_p(cy, t))
    return row


def prior_table(dim, control, U, pdt, start, actions, cells, map_dim, origin, res, v_max, w, dt, pot=None, pot_w=0.0,
                grad_w=0.0, goal_row=None, goal_hash=None):
    """The prior table of one query.  control / U / pdt: the prior's; the rest the searching context's.  cells: the int8
    occupancy map, pot: the potential map or None (both flat, x fastest).  Returns a dict: status, n_steps, T,
    total_cost, pos [n_steps][D], togo [n_steps], goal_row, goal_hash (the given goal when n_steps == 0), steps_t (the t_k),
    taus (the segment ends) and samples: per Command sample (time stamp, |vel|, wrapped cell index, outside, occupied,
    potential value read)."""
    K = _order(control)
    F = 4 * dim + 2
    U = np.asarray(U, dtype=np.float64)
    s = [float(x) for x in np.asarray(start, dtype=np.float64).ravel()]
    segs, taus, status = [], [0.0], 0
    for a in [int(x) for x in np.asarray(actions).ravel()]:
        if a == -1:
            break
        if a < -1 or a >= U.shape[0]:
            status |= BAD_ACTION
            break
        u = [float(x) for x in U[a]]
        cs = _coeffs(dim, K, s, u)
        segs.append((cs, s, u))
        nxt = _waypoint(dim, control, cs, s, u, pdt)
        nxt[4 * dim + 1] = s[4 * dim + 1] + pdt
        s = nxt
        taus.append(pdt + taus[-1])  # trajectory.h:52-56
    S, T = len(segs), taus[-1]
    out = {"status": status, "n_steps": 0, "T": T, "total_cost": 0.0, "pos": np.zeros((0, dim)), "togo": np.zeros(0),
           "goal_row": None if goal_row is None else np.array(goal_row, dtype=np.float64), "goal_hash": goal_hash}
    if S == 0:
        out["status"] |= EMPTY
        return out
    cn = math.ceil(v_max * T / res) if math.isfinite(v_max * T / res) else INF
    if not cn < 2 ** 31:
        out["status"] |= BAD
        return out
    n = int(cn) if cn > 0 else 0
    clamp = lambda tau: min(max(tau, 0.0), T)
    nd = [int(x) for x in map_dim] + [1] * (3 - len(map_dim))
    # traj.sample(n): Command k at k * (T / n) (trajectory.h:230-236, 99-131)
    pts = []
    if n > 0:
        sdt = T / n
        for k in range(n + 1):
            tau = clamp(k * sdt)
            pt, vv = [0.0] * dim, 0.0
            for si in range(S):
                if taus[si] <= tau <= taus[si + 1]:
                    tl = tau - taus[si]
                    for i in range(dim):
                        pt[i] = _p(segs[si][0][i], tl)
                        v = _v(segs[si][0][i], tl) / 1.0
                        vv += v * v
                    break
            pn = [_round_away((pt[i] - origin[i]) / res - 0.5) for i in range(dim)]
            outside = any(pn[i] < 0 or pn[i] >= nd[i] for i in range(dim))
            idx = pn[0] + nd[0] * pn[1] + (nd[0] * nd[1] * pn[2] if dim == 3 else 0)
            idx = _wrap32(idx)
            occupied = (not outside) and int(cells[idx]) == 100
            pv = int(pot[idx]) if (pot is not None and not outside) else 0
            pts.append((k * sdt, math.sqrt(vv), idx, outside, occupied, pv))
    # env_map::traverse_trajectory (env_map.h:229-255)
    traverse, prev = 0.0, -1
    for (_, vn, idx, outside, occupied, pv) in pts:
        if idx == prev:
            continue
        prev = idx
        if outside:
            traverse = INF
            break
        if pot is not None:
            if 0 < pv < 100:
                traverse += pot_w * pv + grad_w * vn
            elif pv >= 100:
                traverse = INF
                break
        elif occupied:
            traverse = INF
            break
    total = traverse + w * T
    costs, ts = [], []
    t = 0.0
    while t < T:  # env_map.h:197-216
        pc = 0.0
        if pot is not None:
            prev = -1
            for (st, vn, idx, outside, occupied, pv) in pts:
                if st >= t:
                    break
                if idx == prev:
                    continue
                prev = idx
                pc += pot_w * pv + grad_w * vn
        costs.append(w * t + pc)
        ts.append(t)
        t += dt
    pos, togo = [], []
    for t in ts:
        k = int(t / dt)  # the truncated quotient, env_map.h:219
        tau = clamp(t)
        for si in range(S):
            if (taus[si] <= tau < taus[si + 1]) or si == S - 1:
                pos.append([_p(segs[si][0][i], tau - taus[si]) for i in range(dim)])
                break
        togo.append(total - costs[k])
    cs, s0, u = segs[-1]
    g = _waypoint(dim, control, cs, s0, u, clamp(T) - taus[S - 1])
    g[4 * dim + 1] = 0.0
    g = [x + 0.0 for x in g]
    out.update(n_steps=len(ts), total_cost=total, pos=np.array(pos, dtype=np.float64).reshape(-1, dim), togo=np.array(togo),
               goal_row=np.array(g), goal_hash=lattice_hash(dim, control, g), steps_t=ts, samples=pts, taus=taus)
    return out


def prior_heur(model, base, dim, s, is_goal_state, prior, dt):
    """Section 3 of include/mplx_prior.h on top of the goal heuristic `base`."""
    if prior is None or prior["n_steps"] == 0 or is_goal_state:
        return base
    t = float(s[4 * dim + 1])
    x = t / dt if t > 0 else 0.0
    if not x < prior["n_steps"]:
        return base
    k = int(x)
    m = max([0.0] + [abs(float(s[i]) - float(prior["pos"][k][i])) for i in range(dim)])
    lin = model.w * m / model.v_max if model.v_max > 0 else model.w * m
    return lin + float(prior["togo"][k])


class PriorOpenModel(OM.OpenModel):
    """OpenModel of one query with a prior (prior_table's dict, or None): the goal is the prior's end."""

    def __init__(self, table, dim, goal_row, goal_hash, w, v_max, dt, prior=None, **kw):
        if prior is not None and prior["n_steps"] > 0:
            goal_row, goal_hash = prior["goal_row"], prior["goal_hash"]
        super().__init__(table, dim, goal_row, goal_hash, w, v_max, **kw)
        self.prior, self.dt = prior, float(dt)

    def heur_and_tol(self, node_id, s):
        h, ok = super().heur_and_tol(node_id, s)
        return prior_heur(self, h, self.dim, s, int(self.table.hash[node_id]) == self.goal_hash, self.prior, self.dt), ok


class PriorMultiOpenModel(MM.MultiOpenModel):
    """MultiOpenModel with priors [Q] (dicts or None): goal rows and hashes are replaced where a prior has steps."""

    def __init__(self, table, dim, goal_rows, goal_hashes, w, v_max, dt, priors, **kw):
        rows = [np.asarray(r, dtype=np.float64) for r in goal_rows]
        hashes = [int(h) for h in goal_hashes]
        for q, p in enumerate(priors):
            if p is not None and p["n_steps"] > 0:
                rows[q], hashes[q] = p["goal_row"], p["goal_hash"]
        super().__init__(table, dim, rows, hashes, w, v_max, **kw)
        self.priors, self.dt = list(priors), float(dt)

    def heur_and_tol(self, node_id, s):
        h, ok = super().heur_and_tol(node_id, s)
        q = self.table.query[node_id]
        return prior_heur(self, h, self.dim, s, int(self.table.hash[node_id]) == self.goal_hashes[q], self.priors[q], self.dt), ok
