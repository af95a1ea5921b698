"""Sequential model of include/mplx_conflict.h: conflicts between K trajectories on a common clock, over positions and an
active mask that the caller supplies, and the stagger loop of motion_primitive_library_amd.search around a callback.

The model does no trajectory arithmetic of its own: tests feed it the positions the device's own sample() returns at the
local times local_times() states (that call is pinned to the reference elsewhere), or closed-form positions of hand
cases.  What it restates is everything after that: who is included, who is active, the pair test in its stated order,
charging by rank, and the four results -- each the minimum the header defines, found by walking the instants in order.
All arithmetic is numpy float64, one IEEE operation per call, in the order of the header."""
import numpy as np

F = np.float64
PARK, GONE = 0, 1
BAD_INPUT = 128


def local_times(step, n_steps, t0, K):
    """[K][n_steps]: tl = (double)i * step - t0[k] (t0 None: tl = (double)i * step)."""
    ti = np.arange(n_steps).astype(F) * F(step)
    if t0 is None:
        return np.broadcast_to(ti[None, :], (K, n_steps)).copy()
    with np.errstate(invalid="ignore"):
        return ti[None, :] - np.asarray(t0, dtype=F)[:, None]


def inputs_ok(K, t0, radius):
    """[K] bool: t0 is finite and the radius is finite and >= 0 (a scalar radius applies to all)."""
    t = np.zeros(K) if t0 is None else np.asarray(t0, dtype=F)
    r = np.broadcast_to(np.asarray(radius, dtype=F), (K,))
    return np.isfinite(t) & np.isfinite(r) & (r >= 0)


def active_mask(tl, total, mode):
    """[n][K] from tl [K][n]: PARK: everywhere; GONE: tl >= 0 && tl <= total."""
    if mode == PARK:
        return np.ones(tl.T.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return ((tl >= 0) & (tl <= np.asarray(total, dtype=F)[:, None])).T


def conflicts(pos, active, radius, included, group=None, rank=None):
    """pos [n][K][D], active [n][K] bool, radius [K] (or a scalar), included [K] bool, group / rank [K] int or None.
    Returns first_step, first_partner [K] int32, min_d2 [K], pair_first [K][K] int32."""
    pos = np.asarray(pos, dtype=F)
    n, K, D = pos.shape
    inc = np.asarray(included, dtype=bool)
    r = np.where(inc, np.broadcast_to(np.asarray(radius, dtype=F), (K,)), 0.0)
    grp = np.arange(K) if group is None else np.asarray(group)
    elig = inc[:, None] & inc[None, :] & (grp[:, None] != grp[None, :]) & ~np.eye(K, dtype=bool)
    # charged[a][b]: the pair is charged to a
    charged = elig if rank is None else elig & (np.asarray(rank)[None, :] <= np.asarray(rank)[:, None])
    rr = r[:, None] + r[None, :]
    rr2 = rr * rr
    first_step, partner = np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    min_d2 = np.full(K, np.inf)
    pair_first = np.full((K, K), -1, np.int32)
    for i in range(n):
        p = pos[i]
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = None
            for d in range(D):
                dx = p[:, None, d] - p[None, :, d]
                d2 = dx * dx if d2 is None else d2 + dx * dx
            both = elig & active[i][:, None] & active[i][None, :]
            conf = both & (d2 < rr2)  # (a NaN compares false)
        cand = both & charged & ~np.isnan(d2)
        min_d2 = np.minimum(min_d2, np.where(cand, d2, np.inf).min(axis=1, initial=np.inf))
        pair_first = np.where((pair_first < 0) & conf, np.int32(i), pair_first)
        cc = conf & charged
        hit = cc.any(axis=1) & (first_step < 0)
        first_step[hit] = i
        partner[hit] = np.argmax(cc[hit], axis=1)  # the smallest index among the partners of that instant
    return {"first_step": first_step, "first_partner": partner, "min_d2": min_d2, "pair_first": pair_first}


def n_steps_for(step, t0, total, ok):
    """The smallest count whose instants i * step cover max(t0 + total) over the trajectories without a status."""
    K = len(total)
    t = np.zeros(K) if t0 is None else np.asarray(t0, dtype=F)
    end = np.where(np.asarray(ok, dtype=bool) & np.isfinite(t), t + np.asarray(total, dtype=F), 0.0)
    last = max(float(end.max()) if K else 0.0, 0.0)
    return int(np.ceil(last / step)) + 1


def stagger(positions, K, step, radius, included, rank=None, delay=None, max_rounds=64, group=None, t0=None):
    """The loop of search.stagger.  positions(t0) -> (pos [n][K][D], active [n][K]) for the clock offsets t0: the caller
    samples there (and applies PARK or GONE).  Each round: one conflicts() with rank (default: the index); every
    trajectory with a charged conflict gets `delay` (default 4 * step) added to its t0; stop when none is charged or
    after max_rounds rounds.  Returns t0, resolved [K] bool (not charged in the last call made), rounds."""
    t = np.zeros(K) if t0 is None else np.array(t0, dtype=F)
    rank = np.arange(K) if rank is None else np.asarray(rank)
    add = F(4.0) * F(step) if delay is None else F(delay)
    charged, rounds = np.zeros(K, dtype=bool), 0
    for _ in range(max_rounds):
        pos, active = positions(t)
        res = conflicts(pos, active, radius, included, group=group, rank=rank)
        rounds += 1
        charged = res["first_step"] >= 0
        if not charged.any():
            break
        t = np.where(charged, t + add, t)
    return t, ~charged, rounds
