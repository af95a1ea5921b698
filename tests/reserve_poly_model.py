"""Sequential model of include/mplx_reserve_poly.h: the problems of a polynomial trajectory set against a reservation
table on the table's clock, and the admission rule of the timed shortcut.

The model does no trajectory arithmetic of its own: tests feed it the table Reservations.positions() returns (or one
built by hand) and, through `own_pos`, the positions of the problems at the local times local_time() states -- the
device's own sample() in Command form, which is pinned to the reference elsewhere, or closed forms of hand cases.  What
it restates is everything else: who is excluded, the horizon, the instants of a problem as the SET the header defines
(found by walking every instant of the table), the pair test in its stated order, the hit as a minimum.  instants_scan
restates how the kernel finds the same set, so that the two can be compared.  All arithmetic is numpy float64, one IEEE
operation per call, in the order of the header."""
import numpy as np

F = np.float64
NO_HIT, HORIZON = -1, -2
BAD_INPUT = 128


def local_time(step, i, t_start):
    """tl_i = (double)i * step - t_start."""
    return F(i) * F(step) - F(t_start)


def inputs_ok(t_start, radius):
    """t_start is finite, the radius is finite and >= 0."""
    return bool(np.isfinite(F(t_start)) and np.isfinite(F(radius)) and F(radius) >= 0)


def leaves_horizon(step, n_steps, t_start, total):
    return bool(F(n_steps - 1) * F(step) - F(t_start) < F(total))


def instants(step, n_steps, t_start, total):
    """Every i in [0, n_steps) with tl_i >= 0 && tl_i <= total, closed at both ends."""
    tl = np.arange(n_steps).astype(F) * F(step) - F(t_start)
    with np.errstate(invalid="ignore"):
        return np.nonzero((tl >= 0) & (tl <= F(total)))[0]


def instants_scan(step, n_steps, t_start, total):
    """The kernel's way: a guess from t_start / step, a scan of at most 4 instants for the first with tl_i >= 0, then
    upwards while tl_i <= total."""
    step, ts, total = F(step), F(t_start), F(total)
    x = ts / step
    g = 0
    if x >= 1.0:
        g = int(x) - 1 if x < 2147483647.0 else n_steps
    first = n_steps
    for s in range(4):
        i = g + s
        if i >= n_steps:
            break
        if F(i) * step - ts >= 0.0:
            first = i
            break
    out = []
    for i in range(first, n_steps):
        tl = F(i) * step - ts
        if not (tl >= 0.0 and tl <= total):
            break
        out.append(i)
    return np.array(out, dtype=np.int64)


def pair_conflicts(p, pos_i, on, rr2):
    """[B] bool: the pair test of one position p [D] against the reservations of one instant, pos_i [D][B]."""
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = None
        for d in range(len(p)):
            dx = F(p[d]) - pos_i[d]
            d2 = dx * dx if d2 is None else d2 + dx * dx
        return on & (d2 < rr2)  # (a NaN compares false)


def check(set_status, n_segs, total, t_start, radius, ignore_group, step, res, own_pos, brute=False):
    """set_status [K] (the set's status bits), n_segs [K], total [K] (the scaled total where the problem holds a Lambda),
    t_start [K], radius [K] or a scalar, ignore_group [K] or None (-1 each); res: the dict of Reservations.positions()
    (pos [n_steps][D][B], active [n_steps][B], included, radius, group [B]); own_pos(k, i, tl) -> [D]: the position of
    problem k at instant i, local time tl.  brute: look at every (i, b) and take the minimum of the keys instead of
    stopping at the first instant with a conflict.  Returns (hit [K] int64, status [K] uint8, n_hit)."""
    K = len(set_status)
    pos, act = np.asarray(res["pos"], dtype=F), np.asarray(res["active"]) != 0
    inc, r_b, g_b = np.asarray(res["included"]) != 0, np.asarray(res["radius"], dtype=F), np.asarray(res["group"])
    n_steps = pos.shape[0]
    rad = np.broadcast_to(np.asarray(radius, dtype=F), (K,))
    ign = np.full(K, -1, np.int64) if ignore_group is None else np.broadcast_to(np.asarray(ignore_group), (K,))
    hit = np.full(K, NO_HIT, np.int64)
    status = np.asarray(set_status, dtype=np.uint8).copy()
    for k in range(K):
        ok = inputs_ok(t_start[k], rad[k])
        if not ok:
            status[k] |= BAD_INPUT
        if set_status[k] != 0 or n_segs[k] == 0 or not ok:
            continue
        if leaves_horizon(step, n_steps, t_start[k], total[k]):
            hit[k] = HORIZON
            continue
        on_k = inc & (g_b != ign[k])
        rr = F(rad[k]) + r_b
        rr2 = rr * rr
        keys = []
        for i in instants(step, n_steps, t_start[k], total[k]):
            p = np.asarray(own_pos(k, int(i), local_time(step, i, t_start[k])), dtype=F)
            conf = pair_conflicts(p, pos[i], on_k & act[i], rr2)
            if brute:
                keys += [(int(i) << 32) | int(b) for b in np.nonzero(conf)[0]]
            elif conf.any():
                hit[k] = (int(i) << 32) | int(np.argmax(conf))
                break
        if brute and keys:
            hit[k] = min(keys)
    return hit, status, int((hit != NO_HIT).sum())


def from_pair_first(pair_first, cand, reserved):
    """What hit must be for candidates and reservations put into ONE set with mode GONE (tests/conflict_model.py or
    PolyTrajSet.conflicts(want_pairs=True)): min over the reserved b with a conflict of (pair_first[k][b] << 32 | index
    of b among `reserved`); -1 without one."""
    out = np.full(len(cand), NO_HIT, np.int64)
    for n, k in enumerate(cand):
        keys = [(int(pair_first[k][b]) << 32) | j for j, b in enumerate(reserved) if pair_first[k][b] >= 0]
        if keys:
            out[n] = min(keys)
    return out


def admit(edge_cost, pair_hit):
    """The timed shortcut's cost matrix from the untimed one: edge_cost [W - 1][max_hop] of one query (+inf: not
    admitted), pair_hit the same shape; a non-adjacent edge (column > 0) with hit != -1 is not admitted."""
    c = np.array(edge_cost, dtype=F)
    block = np.asarray(pair_hit) != NO_HIT
    block[:, 0] = False
    c[block] = np.inf
    return c


def chain_hit(pair_hit, W):
    """The smallest hit >= 0 of the adjacent edges i -> i + 1, i + 1 < W; else -2 if one leaves the horizon; else -1."""
    h = np.asarray(pair_hit)[: max(W - 1, 0), 0]
    if (h >= 0).any():
        return int(h[h >= 0].min())
    return HORIZON if (h == HORIZON).any() else NO_HIT
