"""Sequential model of include/mplx_body.h: the ellipsoid body against a point cloud.

Brute force: no grid, every point against every sample.  What it restates: the shape's derived values, the attitude and
the point test in their stated order, which list entries are looked at, the samples of an edge, the edge's centre and
acceleration as the expression trees of traj::eval_segment (Command form, on the segment traj::chain_segment builds), the
keys and the hit as a minimum, the samples of a trajectory set; and a sequential search whose successor provider is
filtered by the list check.  All arithmetic is numpy float64, one IEEE operation per operator, nothing contracted.
Test infrastructure: nothing shared with the engine."""
import numpy as np

import open_model as OM

F = np.float64
NO_HIT = -1
BAD_ATTITUDE = 0x7fffffff


def shape(r, h, g=9.81, min_cos_tilt=0.0):
    """What mplx_body_set_shape derives, once."""
    r, h, g, m = F(r), F(h), F(g), F(min_cos_tilt)
    R = max(r, h)
    return {"r": r, "h": h, "g": g, "rr": r * r, "hh": h * h, "RR": (R * R) * F(1.0000001), "mct2": m * m}


def _three(x):
    """[D] or [n][D] -> the same with a zero z in 2-D."""
    x = np.asarray(x, dtype=F)
    if x.shape[-1] == 3:
        return x
    return np.concatenate([x, np.zeros(x.shape[:-1] + (1,))], axis=-1)


def attitude(sh, a):
    """(n [3], nn, bad) of an acceleration a [D]."""
    a = _three(a)
    with np.errstate(all="ignore"):
        n = np.array([a[0], a[1], a[2] + sh["g"]], dtype=F)
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        bad = (not n[2] > 0) or bool(n[2] * n[2] < sh["mct2"] * nn)
    return n, nn, bad


def inside(sh, c, a, pts):
    """The point test of every point of pts [n][D] for centre c [D] and acceleration a [D] (whose attitude is good):
    [n] bool."""
    n, nn, bad = attitude(sh, a)
    assert not bad
    c, p = _three(c), _three(np.asarray(pts, dtype=F).reshape(-1, len(np.atleast_1d(c))))
    out = np.zeros(len(p), dtype=bool)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - c[0], p[:, 1] - c[1], p[:, 2] - c[2]
        dd = (dx * dx + dy * dy) + dz * dz
        near = np.nonzero(dd <= sh["RR"])[0]  # (the other conjunct is evaluated for these only: the same AND)
        dx, dy, dz, dd = dx[near], dy[near], dz[near], dd[near]
        dn = (dx * n[0] + dy * n[1]) + dz * n[2]
        a2 = dn * dn / nn
        perp2 = dd - a2
        e = perp2 / sh["rr"] + a2 / sh["hh"]
        out[near] = e <= F(1.0)
    return out


def pair_key(sh, c, a, pts):
    """The low word of a sample's key: BAD_ATTITUDE, the smallest index of a point inside, or NO_HIT."""
    if attitude(sh, a)[2]:
        return BAD_ATTITUDE
    hit = np.nonzero(inside(sh, c, a, pts))[0]
    return int(hit[0]) if len(hit) else NO_HIT


# ---- the edge: traj::chain_segment (dev::Ax<K>::init) and traj::eval_segment<COMMAND, all rows> with lambda = 1
def segment(dim, K, row, u):
    """[D] tuples (c1 .. c5) of the segment from the state row [4D+2] under the control row u."""
    row = np.asarray(row, dtype=F)
    out = []
    for i in range(dim):
        p, v, a, j, ui = row[i], row[dim + i], row[2 * dim + i], row[3 * dim + i], F(u[i])
        z = F(0.0)
        c = {1: (z, z, z, ui, p), 2: (z, z, ui, v, p), 3: (z, ui, a, v, p), 4: (ui, j, a, v, p)}[K]
        out.append(c)
    return out


def eval_segment(seg, t):
    """(pos [D], acc [D]) at local time t."""
    t = F(t)
    lam, lam_dot = F(1.0), F(0.0)
    pos, acc = [], []
    with np.errstate(all="ignore"):
        t3 = (t * t) * t
        t4 = t3 * t
        for c1, c2, c3, c4, c5 in seg:
            pos.append(((((F(0.0) + c1 / F(24) * t4) + c2 / F(6) * t3) + c3 / F(2) * t * t) + c4 * t) + c5)
            v = (((F(0.0) + c1 / F(6) * t3) + c2 / F(2) * t * t) + c3 * t) + c4
            a = ((F(0.0) + c1 / F(2) * t * t) + c2 * t) + c3
            vel = v / lam
            acc.append(a / lam / lam - vel * lam_dot / lam / lam / lam)
    return np.array(pos, dtype=F), np.array(acc, dtype=F)


def sample_times(dt, n_samp):
    ds = F(dt) / F(n_samp)
    return [F(i) * ds for i in range(n_samp)] + [F(dt)]


def check(sh, cloud, count, action, cost, S, parent_id, parent_state, U, dim, K, dt, n_samp):
    """mplx_body_check_device.  cloud [n][D]; count [n_nodes], action / cost [n_nodes * S] (cost is not modified),
    parent_id [n_nodes], parent_state [4D+2][>= n_nodes], U [nU][>= D].
    Returns (cost_out, hit [n_nodes * S] int64, n_blocked, looked [n_nodes * S] bool)."""
    n_nodes, nU = len(count), len(U)
    cloud = np.asarray(cloud, dtype=F).reshape(-1, dim)
    cost = np.asarray(cost, dtype=F)
    out = cost.copy()
    hit = np.full(n_nodes * S, NO_HIT, np.int64)
    looked = np.zeros(n_nodes * S, dtype=bool)
    times = sample_times(dt, n_samp)
    n_blocked = 0
    for k in range(n_nodes):
        if parent_id[k] < 0:
            continue
        for j in range(min(int(count[k]), S)):
            e = k * S + j
            if not np.isfinite(cost[e]) or not 0 <= action[e] < nU:
                continue
            looked[e] = True
            seg = segment(dim, K, np.asarray(parent_state)[:, k], U[int(action[e])])
            for i, s in enumerate(times):
                c, a = eval_segment(seg, s)
                low = pair_key(sh, c, a, cloud)
                if low != NO_HIT:
                    hit[e] = (i << 32) | low
                    break
            if hit[e] != NO_HIT:
                out[e] = np.inf
                n_blocked += 1
    return out, hit, n_blocked, looked


# ---- trajectory sets
def poly_times(step, total):
    """The local times of a problem: i * step while <= total, then total itself (index one past the largest i)."""
    step, total = F(step), F(total)
    out, i = [], 0
    while F(i) * step <= total:
        out.append(F(i) * step)
        i += 1
    return out + [total]


def check_poly(sh, cloud, dim, pos, acc):
    """One problem whose samples (Command form, at poly_times) are pos [n_i][D] and acc [n_i][D]: the hit."""
    cloud = np.asarray(cloud, dtype=F).reshape(-1, dim)
    for i in range(len(pos)):
        low = pair_key(sh, pos[i], acc[i], cloud)
        if low != NO_HIT:
            return (i << 32) | low
    return NO_HIT


# ---- the loop of EnvMap.search(body=) on tests/open_model.py
def filtered(provider, sh, cloud, U, dim, K, dt, n_samp, stats=None):
    """The provider whose lists went through the check: blocked entries cost +inf, which the relax skips."""
    def wrapped(states):
        states = np.asarray(states, dtype=F)
        lists = provider(states)
        n = states.shape[1]
        cost, _, nb, looked = check(sh, cloud, lists["count"], lists["action"], lists["cost"], int(lists["stride"]),
                                    np.zeros(n, np.int32), states, U, dim, K, dt, n_samp)
        lists["cost"] = cost
        if stats is not None:
            stats["blocked"] = stats.get("blocked", 0) + nb
            stats["looked"] = stats.get("looked", 0) + int(looked.sum())
        return lists
    return wrapped


def search(table, opn, provider, sh, cloud, U, dim, K, dt, n_samp, start, start_hash, eps, delta, capacity, stats=None, **kw):
    return OM.search(table, opn, filtered(provider, sh, cloud, U, dim, K, dt, n_samp, stats), start, start_hash, eps, delta,
                     capacity, **kw)
