"""Sequential model of include/mplx_reserve.h (the check of successor lists against a reservation table) and of the
time keys of include/mplx_table.h.

The model does no trajectory arithmetic of its own beyond the forward primitive of hand cases (primitive_pos, the
expression of traj::eval_segment): tests feed it the table Reservations.positions() returns and, through `edge_pos`, the
device's own traj_sample positions of the edges, or closed forms.  What it restates is everything else: which entries
are looked at, the instants of an edge as the SET the header defines (found by walking every instant of the table),
the horizon, the pair test in its stated order, the hit as a minimum.  instants_scan restates how the kernel finds the
same set, so that the two can be compared.  All arithmetic is numpy float64, one IEEE operation per call."""
import math

import numpy as np

F = np.float64
NO_HIT, HORIZON = -1, -2


def instants(step, n_steps, t0, tp, tc):
    """Every i in [0, n_steps) with tl_i = (double)i * step - t0 in [tp, tc], closed at both ends."""
    tl = np.arange(n_steps).astype(F) * F(step) - F(t0)
    with np.errstate(invalid="ignore"):
        return np.nonzero((tl >= F(tp)) & (tl <= F(tc)))[0]


def instants_scan(step, n_steps, t0, tp, tc, dt):
    """The kernel's way: a guess from (tp + t0) / step, then at most ceil(dt / step) + 3 instants."""
    step, t0, tp, tc = F(step), F(t0), F(tp), F(tc)
    n_scan = int(min(math.ceil(F(dt) / step) + 3.0, 2147483647.0))
    x = (tp + t0) / step
    g = 0
    if x >= 1.0:
        g = int(x) - 1 if x < 2147483647.0 else n_steps
    out = []
    for s in range(n_scan):
        i = g + s
        if i >= n_steps:
            break
        tl = F(i) * step - t0
        if tl > tc:
            break
        if tl >= tp:
            out.append(i)
    return np.array(out, dtype=np.int64)


def leaves_horizon(step, n_steps, t0, tc):
    return bool(F(n_steps - 1) * F(step) - F(t0) < F(tc))


def primitive_pos(p, v, a, j, u, order, t):
    """Position of the forward primitive of control order 1 .. 4 from (p, v, a, j) under input u at time t, per axis:
    traj::eval_segment without c0, operation for operation."""
    p, v, a, j, u, t = (np.asarray(x, dtype=F) for x in (p, v, a, j, u, t))
    z = np.zeros_like(p)
    c1, c2, c3, c4, c5 = z, z, z, z, p
    if order == 1:
        c4 = u
    elif order == 2:
        c4, c3 = v, u
    elif order == 3:
        c4, c3, c2 = v, a, u
    elif order == 4:
        c4, c3, c2, c1 = v, a, j, u
    else:
        raise ValueError(order)
    t3 = (t * t) * t
    t4 = t3 * t
    return ((((F(0.0) + c1 / F(24) * t4) + c2 / F(6) * t3) + c3 / F(2) * t * t) + c4 * t) + c5


def check(count, action, cost, S, parent_id, parent_t, dt, n_actions, step, n_steps, res, queries, edge_pos, row_query=None):
    """count [n], action / cost [n * S] (cost is not modified), parent_id / parent_t [n]; res: the dict of
    Reservations.positions() (pos [n_steps][D][B], active [n_steps][B], included, radius, group [B]); queries: (t0 [Q],
    radius [Q], ignore [Q]); row_query [n] or None (all 0; an entry outside [0, Q) makes the row not looked at);
    edge_pos(k, j, i, s) -> [D]: the position of entry (k, j) at instant i, s = tl_i - tp.
    Returns (cost_out [n * S], hit [n * S] int64, n_blocked, looked [n * S] bool)."""
    n = len(count)
    q_t0, q_r, q_ign = (np.asarray(x) for x in queries)
    Q = len(q_t0)
    cost = np.asarray(cost, dtype=F)
    out = cost.copy()
    hit = np.full(n * S, NO_HIT, np.int64)
    looked = np.zeros(n * S, dtype=bool)
    pos, act = np.asarray(res["pos"], dtype=F), np.asarray(res["active"]) != 0
    inc, r_b, g_b = np.asarray(res["included"]) != 0, np.asarray(res["radius"], dtype=F), np.asarray(res["group"])
    D = pos.shape[1]
    n_blocked = 0
    for k in range(n):
        if parent_id[k] < 0:
            continue
        q = 0 if row_query is None else int(row_query[k])
        if q < 0 or q >= Q:
            continue
        tp = F(parent_t[k])
        tc = tp + F(dt)
        off = leaves_horizon(step, n_steps, q_t0[q], tc)
        ii = [] if off else instants(step, n_steps, q_t0[q], tp, tc)
        on_q = inc & (g_b != q_ign[q])
        rr = F(q_r[q]) + r_b
        rr2 = rr * rr
        for j in range(min(int(count[k]), S)):
            e = k * S + j
            if not np.isfinite(cost[e]) or not (0 <= action[e] < n_actions):
                continue
            looked[e] = True
            if off:
                hit[e] = HORIZON
            for i in ii:
                tl = F(i) * F(step) - F(q_t0[q])
                p = np.asarray(edge_pos(k, j, int(i), tl - tp), dtype=F)
                with np.errstate(invalid="ignore", over="ignore"):
                    d2 = None
                    for d in range(D):
                        dx = p[d] - pos[i, d]
                        d2 = dx * dx if d2 is None else d2 + dx * dx
                    conf = on_q & act[i] & (d2 < rr2)  # (a NaN compares false)
                if conf.any():
                    hit[e] = (int(i) << 32) | int(np.argmax(conf))
                    break
            if hit[e] != NO_HIT:
                out[e] = np.inf
                n_blocked += 1
    return out, hit, n_blocked, looked


# ---- time keys (include/mplx_table.h): the last hash_combine of Waypoint::enable_t
MASK = (1 << 64) - 1


def round_half_away(x):
    """std::round: half away from zero (Python's round is half to even)."""
    a = abs(x)
    f = math.floor(a)
    r = f + (1 if a - f >= 0.5 else 0)  # (a - f is exact)
    return int(math.copysign(r, x))


def hash_combine(seed, value):
    """boost::hash_combine (< 1.81) with hash_value(int) = the sign-extending conversion."""
    return (seed ^ (((value & MASK) + 0x9E3779B9 + ((seed << 6) & MASK) + (seed >> 2)) & MASK)) & MASK


def time_key(h, t):
    """combine(hash, (int)std::round(t / 0.1)); t / 0.1 is one IEEE division."""
    return hash_combine(int(h), round_half_away(float(F(t) / F(0.1))))
