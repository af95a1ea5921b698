"""The model mplx_shortcut (include/mplx_limits.h) is compared with: the dynamic programme over the hops of one chain, a
brute force over every chain of hops, and the edge costs of a pair set from the coefficients the device returned.

Costs of a chain of W states: c[i][h] is the cost of the hop i -> i + h + 1 (h < max_hop), +inf where the hop is not
admitted, NaN on an adjacent hop whose solve failed (a bad chain).  dist[0] = 0.0, dist[j] = min over max(0, j - max_hop)
<= i < j of dist[i] + c[i][j - i - 1], one add per candidate, ties to the smallest i."""
import functools
import itertools

import numpy as np

import limits_model as LM
import solve_model as SM
import traj_model as TM

EMPTY, BAD_CHAIN = 1, 16
F = np.float64


def dp(c, W, max_hop):
    """(status, keep, cost, chain_cost) of one chain; c [>= W - 1][max_hop]."""
    if W < 2:
        return EMPTY, [], F(np.nan), F(np.nan)
    adjacent = [F(c[i][0]) for i in range(W - 1)]
    if any(np.isnan(e) for e in adjacent):
        return BAD_CHAIN, list(range(W)), F(np.nan), F(np.nan)
    chain = F(0.0)
    for e in adjacent:
        chain = chain + e
    dist, pred = [F(0.0)], [-1]
    for j in range(1, W):
        best, bi = F(np.inf), j - 1
        for i in range(max(0, j - max_hop), j):
            v = dist[i] + F(c[i][j - i - 1])
            if v < best:
                best, bi = v, i
        dist.append(best)
        pred.append(bi)
    keep, j = [], W - 1
    while j >= 0:
        keep.append(j)
        j = pred[j]
    return 0, keep[::-1], dist[W - 1], chain


def brute(c, W, max_hop):
    """Every ascending chain 0 .. W - 1 with hops <= max_hop: the cheapest (costs added from the left), ties to the chain
    whose reversed index list is smallest -- the programme's rule when the sums are exact."""
    best = None
    for r in range(W - 1):
        for mid in itertools.combinations(range(1, W - 1), r):
            chain = (0,) + mid + (W - 1,)
            if any(b - a > max_hop for a, b in zip(chain, chain[1:])):
                continue
            total = F(0.0)
            for a, b in zip(chain, chain[1:]):
                total = total + F(c[a][b - a - 1])
            key = (total, chain[::-1])
            if best is None or key < best:
                best = key
    return list(best[1][::-1]), best[0]


def edge_costs(pairs, max_hop, D, so, control, w, limits, world, want_detail=False):
    """c of every pair from what the device holds in `pairs` (coefficients, yaw, dts, status): [P], pair p = (k (w_max - 1)
    + i) max_hop + (j - i - 1).  limits = (v_max,
    a_max, j_max); world = (grid, pot or None, md, org, res, v_max, pot_w, grad_w) of traj_model.traverse.  `control` may
    carry the yaw bit: it adds nothing to the validity (myaw = 0) and the effort row is `so`, the control's own order.
    want_detail: also near [P] (a non-adjacent pair one of whose ALL_ROOTS maxima of a checked limit lies within a
    relative NEAR of that limit: its validity may turn on the last bits of cbrt / acos / cos) and trav [P] (the traversal
    cost as it is, before an adjacent edge counts a non-finite one as 0.0)."""
    coef, yaw, dts, status = pairs.coefficients(), pairs.yaw_coefficients(), pairs.dts(), pairs.status
    P = pairs.n
    out, near, travs = np.zeros(P), np.zeros(P, bool), np.full(P, np.nan)
    lim = [F(x) for x in limits]
    checked = [q for q, c in enumerate(LM.checks_of(control)) if c and not lim[q] <= 0]
    for p in range(P):
        adjacent = p % max_hop == 0
        if status[p]:
            out[p] = np.nan if adjacent else np.inf
            continue
        tr = SM.PolySet(coef[:1, :, :, p].reshape(-1, D), yaw[:1, :, p].reshape(-1), dts[:1, p], so, D)
        trav = F(TM.traverse(tr, *world)["cost"])
        travs[p] = trav
        base = tr.effort[so] + F(w) * F(tr.T)
        if adjacent:
            out[p] = base + (trav if np.isfinite(trav) else F(0.0))
        else:
            lm = LM.traj_limits([tr.coef[0]], tr.dts, control, *limits, LM.ALL_ROOTS)
            out[p] = base + trav if (lm["valid"] == 1 and np.isfinite(trav)) else np.inf
            for q in checked:
                m = lm[("max_vel", "max_acc", "max_jrk")[q]]
                near[p] = near[p] or bool((np.abs(m - lim[q]) <= NEAR * lim[q]).any())
    return (out, near, travs) if want_detail else out


NEAR = 1e-9  # far above the 8 * 2^-52 the limits tests hold the device's cbrt / acos / cos to


def pair_problem(states, k, i, j, D):
    """The two-waypoint reference problem of pair (k, i, j) of chain states [4D+2][W][Q]: (vals [3][2][D], flags [2] = 7,
    7: every derivative fixed at both ends, dts [1] = t_j - t_i by one IEEE subtraction, yaw [2]) as solve_model's
    solve_dense / solve_exact / yaw_solve take them."""
    vals = np.stack([states[a * D:(a + 1) * D, [i, j], k].T for a in range(3)])
    dts = np.array([F(states[4 * D + 1, j, k]) - F(states[4 * D + 1, i, k])])
    return vals, np.array([7, 7], np.uint8), dts, states[4 * D, [i, j], k].copy()


def pair_index(k, i, j, w_max, max_hop):
    return (k * (w_max - 1) + i) * max_hop + (j - i - 1)


class DensePairs:
    """What edge_costs reads of a device pair set, from solve_dense instead: the CPU stand-in for tuning and for the checks
    of the batch that need no GPU."""

    def __init__(self, states, n_wp, D, so, max_hop):
        W, Q = states.shape[1], states.shape[2]
        N = 2 * (so + 1)
        self.n = Q * (W - 1) * max_hop
        self.status = np.ones(self.n, np.uint8)
        self._c, self._y, self._d = np.zeros((1, N, D, self.n)), np.zeros((1, 2, self.n)), np.zeros((1, self.n))
        for k in range(Q):
            Wk = min(int(n_wp[k]), W)
            for i in range(Wk - 1):
                for j in range(i + 1, min(i + max_hop, Wk - 1) + 1):
                    p = pair_index(k, i, j, W, max_hop)
                    vals, flags, dts, yaw = pair_problem(states, k, i, j, D)
                    if not (np.isfinite(dts[0]) and dts[0] > 0):
                        self.status[p] = SM.S_BAD_TIME
                        continue
                    self.status[p] = 0
                    self._c[0, :, :, p], self._d[0, p] = SM.solve_dense(vals, flags, dts, so), dts[0]
                    self._y[0, :, p] = SM.yaw_solve(yaw, dts)[:, 0]

    def coefficients(self):
        return self._c

    def yaw_coefficients(self):
        return self._y

    def dts(self):
        return self._d


# ------------------------------------------------------------------------------------------------------- the batch
Q, WMAX, HOP = 67, 6, 3
W_TIME, POT_W, GRAD_W = 10.0, 0.1, 0.25
MAPS = {2: ([40, 40], [0.0, 0.0], 0.25), 3: ([24, 21, 19], [-1.0, 0.5, -0.3], 0.25)}
LINE_X0 = {2: 2.5, 3: -0.5}                           # the line queries: x = x0 + w, one metre and one second apart
LINE_LOW, LINE_HIGH = {2: [2.0], 3: [2.0, 2.0]}, {2: [8.0], 3: [5.0, 1.0]}  # y (, z): through the wall / clear of it
OFF_Y = {2: 10.3, 3: 6.0}                             # a y past the map's edge
TIE, REPEAT_T, WALL, OFF_MAP = (6, 63), (14,), (22, 66), (30,)
# (D, control) -> (v_max, a_max): chosen on the CPU (DensePairs) so that the programme has something to decide
# (ACC: the line queries move at exactly v_max, an IEEE-only decision; JRK: v_max is kept away from their speed, so that
# they do not use up the pairs the test may leave out)
CONFIGS = {(2, 0x01): (2.0, 1.5), (3, 0x01): (2.0, 1.5), (2, 0x03): (1.0, 1.5), (3, 0x03): (1.0, 1.5), (2, 0x07): (1.25, 1.0),
           (3, 0x07): (1.25, 1.0), (2, 0x13): (1.0, 1.5), (3, 0x17): (1.25, 1.0)}


def has_potential(D, control):
    return D == 3 and (control & 0x0F) >= 0x03


@functools.lru_cache(maxsize=None)
def batch_states(D):
    """states [4D+2][WMAX][Q] and n_wp [Q] = k % 8 of the batch, computed once and never changed; which k is what: the
    docstring of tests/test_gpu_shortcut.py."""
    md, org, res = MAPS[D]
    rng = np.random.default_rng(900 + D)
    lo, hi = np.asarray(org) + 0.4, np.asarray(org) + np.asarray(md) * res - 0.4
    st = np.zeros((4 * D + 2, WMAX, Q))
    for k in range(Q):
        while True:
            pos = np.zeros((WMAX, D))
            pos[0] = np.round(rng.uniform(lo, hi), 3)
            d = rng.uniform(-1, 1, D)
            d = d / np.linalg.norm(d)
            for w in range(1, WMAX):
                pos[w] = pos[w - 1] + np.round(d * rng.uniform(0.3, 0.7) + rng.uniform(-0.15, 0.15, D), 3)
            if (pos >= lo).all() and (pos <= hi).all():
                break
        t = np.concatenate([[0.0], np.cumsum(rng.integers(4, 9, WMAX - 1) / 8.0)]) + rng.integers(0, 16) / 8.0
        vel = np.zeros_like(pos)
        for w in range(WMAX):
            a, b = max(w - 1, 0), min(w + 1, WMAX - 1)
            vel[w] = (pos[b] - pos[a]) / (t[b] - t[a])
        st[0:D, :, k] = pos.T
        st[D:2 * D, :, k] = np.round(vel + rng.uniform(-0.05, 0.05, vel.shape), 2).T
        st[2 * D:3 * D, :, k] = np.round(rng.uniform(-0.2, 0.2, (D, WMAX)), 2)
        st[3 * D:4 * D, :, k] = np.round(rng.uniform(-0.5, 0.5, (D, WMAX)), 2)
        st[4 * D, :, k] = rng.uniform(-3, 3, WMAX)
        st[4 * D + 1, :, k] = t

    def line(k, rest, xs=None):
        st[:, :, k] = 0.0
        st[0, :, k] = LINE_X0[D] + (np.arange(WMAX) if xs is None else np.asarray(xs, float))
        st[1:D, :, k] = np.asarray(rest)[:, None]
        st[D, :, k] = 1.0
        st[4 * D, :, k] = 0.1 * np.arange(WMAX) - 0.2
        st[4 * D + 1, :, k] = np.arange(WMAX)

    for k in TIE + OFF_MAP:
        line(k, LINE_HIGH[D])
    line(WALL[0], LINE_LOW[D])
    line(WALL[1], LINE_LOW[D], xs=[2, 3, 4, 5, 4, 3])  # W = 2: its only piece, state 0 -> 1, goes through the wall
    st[1, 3, OFF_MAP[0]] = OFF_Y[D]
    for k in REPEAT_T:
        st[4 * D + 1, 3, k] = st[4 * D + 1, 2, k]
    st.setflags(write=False)
    n_wp = (np.arange(Q) % 8).astype(np.int32)
    n_wp.setflags(write=False)
    return st, n_wp


@functools.lru_cache(maxsize=None)
def batch(D, control):
    """The inputs of one configuration: dict(states, n_wp, grid, pot (or None), map = (md, org, res), v_max, a_max, so,
    world (traj_model.traverse's), limits (limits_model.traj_limits's))."""
    md, org, res = MAPS[D]
    st, n_wp = batch_states(D)
    if D == 2:
        grid = np.zeros((40, 40), np.int8)
        grid[0:24, 19:21] = 100  # x in [4.75, 5.25), y in [0, 6)
    else:
        grid = np.zeros((19, 21, 24), np.int8)
        grid[:, 0:12, 11:13] = 100  # x in [1.75, 2.25), y in [0.5, 3.5), every z
    pot = None
    if has_potential(D, control):
        pot = np.random.default_rng(77).integers(0, 60, grid.shape).astype(np.int8)
        pot[grid == 100] = 100
        pot = pot.ravel().copy()
    grid = grid.ravel().copy()
    v_max, a_max = CONFIGS[(D, control)]
    return {"states": st, "n_wp": n_wp, "grid": grid, "pot": pot, "map": (md, org, res), "v_max": v_max, "a_max": a_max,
            "so": SM.so_of(control), "world": (grid, pot, md, org, res, v_max, POT_W, GRAD_W), "limits": (v_max, a_max, 0.0)}


def w_of(n_wp, k):
    return min(int(n_wp[k]), WMAX)  # a count above w_max behaves as w_max
