"""The slit of tests/test_body_model.py (CPU, on the model) and tests/test_gpu_body.py (the device against the model).

3-D ACC, controls {-10, 0, 10}^2 x {0}, dt = 0.2, an all-free voxel map of 4 m x 2 m x 0.4 m that confines the search.
The obstacle is in the cloud alone: a wall at x = 2 over the map's whole width and more than its height, points 0.05 m
apart, with a full-height slit of half-width W around y = 1 (the first points stand at exactly 1 -/+ W).  The body is a
flat disc, r = 0.3 and h = 0.05: upright its half-width across the slit is 0.3 > W; rolled by atan(10 / 9.81) it is
sqrt(0.09 cos^2 + 0.0025 sin^2) = 0.213 < W, and with v_y = -/+ 1 at the chain states an a_y that alternates between +10
and -10 keeps |y - 1| <= 0.05 while v_x carries the disc through.  A sphere r = h = 0.3 is as wide whatever its
attitude and the map leaves no way round: it finds no path."""
import numpy as np

import body_model as BM
import open_model as OM
from table_model import TableModel, oracle_provider

W = 0.28
FLAT, BALL = (0.3, 0.05), (0.3, 0.3)
N_SAMP = 4
CAP = 1 << 13
# the model's numbers, recorded from tests/test_body_model.py: (status, cost, rounds, expanded, actions) and, for the
# sphere, (rounds, expanded) of the search that runs empty
SLIT_FLAT_MODEL = (OM.FOUND, 114.0, 38, 430, [7, 5, 4, 3, 5, 4, 3])  # +x, then a_y = +10 / 0 / -10 / +10 / 0 / -10 at v_x = 2
SLIT_BALL_MODEL = (47, 472)


# ---- the list check: cases a .. g of tests/test_gpu_body.py, built and run through the model once
# name -> (dim, control, axis values, yaw, S, rows, points, n_samp, r, h, min_cos_tilt, extras); r and h are dyadic, so
# that a point r beside a dyadic centre lies exactly on the surface; they are sized on the CPU so that the model blocks
# between 10 % and 90 % of the looked-at entries.  extras: "edge" points within an ulp of cell boundaries (the grid's
# origin is pinned to 0 by a corner point), "far" outliers that force the edge doubling.
THREE = [-4.0, 0.0, 4.0]
NINE = [-4.0, -3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0]
LIST_CASES = {
    "a": (3, "ACC", THREE, False, 27, 5, 1, 1, 0.5, 0.25, 0.0, ()),
    "b": (3, "ACC", THREE, False, 32, 67, 70, 4, 0.5, 0.25, 0.0, ("edge",)),
    "c": (3, "JRK", THREE, False, 27, 130, 4097, 8, 0.125, 0.0625, 0.0, ("edge",)),
    "d": (3, "VEL", THREE, False, 27, 67, 257, 4, 0.375, 0.25, 0.0, ("edge",)),
    "e": (2, "ACC", NINE, False, 96, 67, 257, 4, 0.0625, 0.03125, 0.0, ("edge",)),
    "f": (3, "ACCxYAW", THREE, True, 81, 9, 70, 4, 0.5, 0.25, 0.0, ("far",)),
    "g": (3, "ACC", None, False, 27, 37, 20, 4, 0.5, 0.25, 0.8, ("far",)),
}
ORDER = {"VEL": 1, "ACC": 2, "JRK": 3, "ACCxYAW": 2}
G = 9.81
DT = 1.0
_cache = {}


def auto_edge(r, h, mult=1):
    """The cell edge mplx_body_set_shape derives (libm's sqrt is correctly rounded on both sides)."""
    import math
    R = max(np.float64(r), np.float64(h))
    return math.sqrt(float((R * R) * np.float64(1.0000001))) * 1.000001 * float(mult)


def list_case(name):
    """Everything of one case, and what the model makes of it: a dict.  Built once per name."""
    if name in _cache:
        return _cache[name]
    dim, control, vals, yaw, S, n, n_pts, n_samp, r, h, mct, extras = LIST_CASES[name]
    rng = np.random.default_rng(ord(name))
    K = ORDER[control]
    import itertools
    if vals is None:  # case g: the third axis decides the attitude
        rows = [[x, y, z] for x in (-8.0, 0.0, 8.0) for y in (-8.0, 0.0, 8.0) for z in (-12.0, 0.0, 12.0)]
    else:
        rows = [list(c) for c in itertools.product(vals, repeat=dim)]
    if yaw:
        rows = [c + [y] for c in rows for y in (-0.3, 0.0, 0.3)]
    U = np.array(rows, dtype=np.float64)
    nU, F = len(U), 4 * dim + 2
    n_alloc = n + 3
    # ---- parents: row 0 at a dyadic position and at rest, the others anywhere in [2, 6]^D
    pst = np.zeros((F, n_alloc))
    pst[:dim, :n] = rng.uniform(2.0, 6.0, size=(dim, n))
    if K >= 2:
        pst[dim:2 * dim, :n] = rng.uniform(-0.5, 0.5, size=(dim, n))
    if K >= 3:
        pst[2 * dim:3 * dim, :n] = rng.uniform(-3.0, 3.0, size=(dim, n))
    if yaw:
        pst[4 * dim, :n] = rng.uniform(-3.0, 3.0, size=n)
    pst[F - 1, :n] = np.arange(n) * 0.5
    pst[:4 * dim, 0] = 0.0
    pst[:dim, 0] = [3.0, 4.0, 2.5][:dim]
    if name == "a":  # one point: row 3 ends on it under +x, row 4 passes it by
        pst[:, 3], pst[:, 4] = pst[:, 0], pst[:, 0]
        pst[0, 3], pst[1, 4] = pst[0, 0] - 1.75, pst[1, 4] + 3.0
    parent_id = np.arange(n, dtype=np.int32)
    parent_id[[1] + ([20] if n > 20 else [])] = -1
    count = rng.integers(0, min(S, nU) + 1, size=n_alloc).astype(np.int32)
    count[:3] = [min(S, nU), min(S, nU), 0]
    if n > 3:
        count[3:5] = min(S, nU)
    N = n_alloc * S
    live = (np.arange(S)[None, :] < count[:, None]).ravel()
    live[n * S:] = False
    action = np.frombuffer(b"\x5a" * (4 * N), np.int32).copy()
    cost = np.frombuffer(b"\x5a" * (8 * N), np.float64).copy()
    action[live] = rng.integers(0, nU, size=int(live.sum()))
    cost[live] = rng.choice([0.5, 1.0, 2.0, np.inf, np.nan], p=[0.3, 0.3, 0.3, 0.05, 0.05], size=int(live.sum()))
    bad = np.nonzero(live)[0][5::11]
    action[bad[0::2]], action[bad[1::2]] = nU + 3, -1  # out of range
    for k in (0, 3, 4):  # every control once, in order, with finite costs
        if k < n:
            m_ = min(S, nU)
            action[k * S:k * S + m_], cost[k * S:k * S + m_] = np.arange(m_), 1.0
    # ---- the cloud: the surface pair first, then what the case asks for, then random points in the reach
    p0 = pst[:dim, 0]
    on, off = p0.copy(), p0.copy()
    on[0], off[0] = p0[0] + r, np.nextafter(p0[0] + r, np.inf)
    special = [on, off] if n_pts >= 70 else [on]
    if n_pts >= 70:
        nf = np.full(dim, 5.0)
        nf2, nf3 = nf.copy(), nf.copy()
        nf[0], nf2[dim - 1], nf3[1] = np.nan, np.inf, -np.inf
        special += [nf, nf2, nf3]
    if "edge" in extras:
        edge = auto_edge(r, h)
        special.append(np.zeros(dim))  # the corner that pins the grid's origin
        q = pst[:dim, 3].copy()
        kx = np.floor(q[0] / edge)
        for x in (kx * edge, np.nextafter(kx * edge, -np.inf), np.nextafter(kx * edge, np.inf), (kx + 1) * edge):
            b = q.copy()
            b[0] = x
            special.append(b)
        b = q.copy()
        b[1] = np.nextafter(np.floor(q[1] / edge) * edge, -np.inf)
        special.append(b)
    if "far" in extras:
        special += [np.full(dim, 1e6), np.full(dim, -3e9)]
    special = special[:n_pts]
    cloud = np.concatenate([np.array(special).reshape(-1, dim), rng.uniform(0.5, 7.5, size=(n_pts - len(special), dim))])
    sh = BM.shape(r, h, G, mct)
    want_cost, want_hit, want_nb, looked = BM.check(sh, cloud, count[:n], action[:n * S], cost[:n * S], S, parent_id, pst, U, dim, K,
                                                    DT, n_samp)
    out = dict(name=name, dim=dim, control=control, K=K, U=U, nU=nU, S=S, n=n, n_alloc=n_alloc, n_samp=n_samp, r=r, h=h, mct=mct,
               pst=pst, parent_id=parent_id, count=count, action=action, cost=cost, cloud=cloud, sh=sh, want_cost=want_cost,
               want_hit=want_hit, want_nb=want_nb, looked=looked, frac=want_nb / max(int(looked.sum()), 1))
    _cache[name] = out
    return out


def slit(m):
    U = np.array([[ax, ay, 0.0] for ax in (-10.0, 0.0, 10.0) for ay in (-10.0, 0.0, 10.0)])
    dims, res = [40, 20, 4], 0.1
    ys = np.concatenate([1.0 - W - 0.05 * np.arange(20), 1.0 + W + 0.05 * np.arange(20)])
    ys = ys[(ys > -0.2) & (ys < 2.2)]
    zs = -0.2 + 0.05 * np.arange(17)  # -0.2 .. 0.6 around the flight level 0.2
    cloud = np.array([[2.0, y, z] for y in ys for z in zs])
    start = m.Waypoint(3, m.ACC, pos=[0.55, 1.0, 0.2], vel=[0.0, -1.0, 0.0]).to_row()
    goal = m.Waypoint(3, m.ACC, pos=[3.35, 1.0, 0.2]).to_row()
    return {"U": U, "dims": dims, "res": res, "origin": [0.0, 0.0, 0.0], "cells": np.zeros(int(np.prod(dims)), np.int8),
            "dt": 0.2, "v_max": 3.0, "a_max": 10.0, "w": 10.0, "tol_pos": 0.25, "cloud": cloud, "wall_x": 2.0,
            "start": start, "goal": goal}


def slit_env(m, sc):
    env = m.EnvMap(3)
    env.setMap(sc["origin"], sc["dims"], sc["cells"], sc["res"])
    env.set_control(m.ACC)
    env.set_u(sc["U"])
    env.set_v_max(sc["v_max"])
    env.set_a_max(sc["a_max"])
    env.set_dt(sc["dt"])
    return env


def slit_model_search(m, O, sc, rh, max_expand=None):
    """OM.search with the provider filtered by the model's check.  Returns the search's dict, the cost, the path's actions
    and its states' rows [4D+2][len + 1]."""
    oenv = O.Env(3, O.ACC, sc["U"], sc["cells"], sc["dims"], sc["origin"], sc["res"], dt=sc["dt"], w=sc["w"],
                 v_max=sc["v_max"], a_max=sc["a_max"])
    table = TableModel(14)
    opn = OM.OpenModel(table, 3, sc["goal"], O.lattice_hash(3, O.ACC, sc["goal"]), w=sc["w"], v_max=sc["v_max"],
                       tol_pos=sc["tol_pos"])
    sh = BM.shape(rh[0], rh[1])
    stats = {}
    out = BM.search(table, opn, oracle_provider(O, oenv), sh, sc["cloud"], sc["U"], 3, 2, sc["dt"], N_SAMP, sc["start"],
                    O.lattice_hash(3, O.ACC, sc["start"]), 1.0, sc["w"] * sc["dt"], CAP, stats=stats, max_expand=max_expand)
    res = out["result"]
    actions, states, cost = None, None, np.inf
    if out["status"] == OM.FOUND:
        i, actions, ids = int(res["goal_id"]), [], []
        cost = float(res["goal_g"])
        while i >= 0:
            ids.append(i)
            if table.pred[i] >= 0:
                actions.append(int(table.pred_action[i]))
            i = int(table.pred[i])
        actions = actions[::-1]
        states = np.stack([table.state[i] for i in ids[::-1]], axis=1)
    return {"out": out, "cost": cost, "actions": actions, "states": states, "stats": stats, "table": table}
