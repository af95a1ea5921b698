"""Inputs and the CPU reference of the timed shortcut's batch (tests/test_shortcut_timed_cases.py on the CPU,
tests/test_gpu_shortcut_timed_batch.py on the device): the batch of tests/shortcut_model.py -- Q = 67 queries, w_max = 6,
max_hop = 3, n_wp = k % 8, the TIE / REPEATED-T / WALL / OFF-MAP queries -- against a table of stationary reservations.

The table (reservations(D, B)): B one-segment constant trajectories (reserve_poly_cases.line) at positions on the 1/8
grid over the map, radii from RADII[B], groups b // 2, every ninth one S = 0 (a failed load: excluded), t0 in quarters from
0 to 5 and a segment time in quarters (QUARTERS[B]): filled PARK the reservation stands for ever, filled GONE it is there
during [t0, t0 + time] only.  B = 65 (a tile and a lane) is filled PARK, B = 300 (past the kKeep = 4 register tiles of
csrc/reserve_poly_kernel.hip) GONE, with smaller radii and shorter times: with those of B = 65 it blocks nearly every
hop.  Step 0.25, N_STEPS[D] = 23 / 25 instants: the horizon ends at t = 5.5 / 6, which the later chains leave.

The queries (query_rows(D, B)): t0[k] = 0.1 (k % 11) -- but for 0, 0.5 and 1 not a multiple of the step, so t0[k] + t_i
rounds and t_start / step is no integer --, radius[k] from {0.125, 0.25, 0.5} by k % 3, ignore_group[k] = the group of the
included reservation nearest to the chain's states (k % 3 != 0; else -1): the group most likely to be in the chain's way,
so that ignoring it matters.

reference(D, control, B): everything of the model, from shortcut_model.DensePairs (no GPU): the untimed edge costs, the
pair hits (reserve_poly_model.check on the dense pairs' own polynomials), the masked costs, both programmes, chain_hit.
counts(ref) are the conditions that keep the device test from being vacuous."""
import functools

import numpy as np

import reserve_poly_cases as RC
import reserve_poly_model as RPM
import shortcut_model as XM
import solve_model as SM
import traj_model as TM

F = np.float64
STEP, N_STEPS = 0.25, {2: 23, 3: 25}
BS = (65, 300)
PARK = {65: True, 300: False}
RADII = {65: (0.125, 0.25, 0.5), 300: (0.0625, 0.125, 0.25)}
QUARTERS = {65: (2, 17), 300: (1, 7)}  # the segment time, in quarters: [lo, hi)
SEEDS = {(2, 65): 7, (2, 300): 7, (3, 65): 0, (3, 300): 0}  # tried on the CPU: with these every condition of counts() holds
Q, WMAX, HOP = XM.Q, XM.WMAX, XM.HOP
PAD_STRIDE = 71  # the stride of the raw ABI test: what a t row read as [i * Q + k] from it gives is counted


@functools.lru_cache(maxsize=None)
def reservations(D, B):
    """{"res": (c, dts, n_segs) as EnvMap.load_traj takes them, "t0", "r_b", "group" [B], "park"}."""
    md, org, res = XM.MAPS[D]
    rng = np.random.default_rng(7100 + 1000 * D + B + 100000 * SEEDS[(D, B)])
    c, dts, n_segs = RC.line(D, B)
    for d in range(D):
        c[0, d, 5, :] = (np.ceil(org[d] * 8) + rng.integers(1, int(md[d] * res * 8), B)) / 8.0  # (multiples of 1/8: exact)
    dts[0, :] = rng.integers(*QUARTERS[B], B) / 4.0
    n_segs[8::9] = 0
    out = {"res": (c, dts, n_segs), "t0": rng.integers(0, 21, B) / 4.0, "r_b": rng.choice(RADII[B], B),
           "group": (np.arange(B) // 2).astype(np.int32), "park": PARK[B]}
    for a in (c, dts, n_segs, out["t0"], out["r_b"], out["group"]):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def table(D, B):
    """The dict of Reservations.positions() for reservations(D, B), on the host."""
    r = reservations(D, B)
    c, dts, n_segs = r["res"]
    return RC.host_table(c, dts, n_segs, STEP, N_STEPS[D], r["t0"], r["r_b"], r["group"], r["park"])


@functools.lru_cache(maxsize=None)
def query_rows(D, B):
    """(t0, radius, ignore_group), [Q] each."""
    st, n_wp = XM.batch_states(D)
    r = reservations(D, B)
    at = r["res"][0][0, :D, 5, :]  # [D][B]
    inc = r["res"][2] > 0
    t0 = 0.1 * (np.arange(Q) % 11)
    radius = np.array([0.125, 0.25, 0.5])[np.arange(Q) % 3]
    ignore = np.full(Q, -1, np.int32)
    for k in range(Q):
        W = XM.w_of(n_wp, k)
        if k % 3 == 0 or W < 2:
            continue
        d2 = ((st[:D, :W, k][:, :, None] - at[:, None, :]) ** 2).sum(0).min(0)  # [B]: the nearest state of the chain
        ignore[k] = r["group"][np.argmin(np.where(inc, d2, np.inf))]
    for a in (t0, radius, ignore):
        a.setflags(write=False)
    return t0, radius, ignore


def pair_rows(t_rows, t0, radius, ignore, hop, t_at=None):
    """(t_start, radius, ignore) [P] of the pair set, pair p = (k (W - 1) + i) hop + h: t0[k] + t_i by one IEEE add.
    t_rows [W][Q]; t_at(i, k): another way to read the t row (the counterfactuals)."""
    W, n = t_rows.shape
    ts, rad, ign = np.zeros(n * (W - 1) * hop), np.zeros(n * (W - 1) * hop), np.zeros(n * (W - 1) * hop, np.int32)
    for k in range(n):
        for i in range(W - 1):
            p = (k * (W - 1) + i) * hop
            t = t_rows[i, k] if t_at is None else t_at(i, k)
            ts[p:p + hop], rad[p:p + hop], ign[p:p + hop] = F(t0[k]) + F(t), radius[k], ignore[k]
    return ts, rad, ign


@functools.lru_cache(maxsize=None)
def dense(D, control, hop=HOP):
    """(DensePairs, the untimed edge costs [Q][WMAX - 1][hop], the pairs' primitives [P][D][6])."""
    b = XM.batch(D, control)
    so = b["so"]
    dp = XM.DensePairs(b["states"], np.minimum(b["n_wp"], WMAX), D, so, hop)
    cost = XM.edge_costs(dp, hop, D, so, control, XM.W_TIME, b["limits"], b["world"]).reshape(Q, WMAX - 1, hop)
    prim = np.stack([SM.to_primitive_coeffs(dp.coefficients()[0, :, :, p], so)[0] for p in range(dp.n)])
    return dp, cost, prim


def hits(D, control, B, rows, hop=HOP, tab=None):
    """reserve_poly_model.check of the dense pairs with the rows (t_start, radius, ignore) [P]: hit [Q][WMAX - 1][hop]."""
    dp, _, prim = dense(D, control, hop)
    ts, rad, ign = rows
    own = lambda p, i, tl: np.array([TM.poly_p(prim[p, d], F(tl)) for d in range(D)])
    hit, _, _ = RPM.check(dp.status, (dp.status == 0).astype(np.int32), dp.dts()[0], ts, rad, ign, STEP,
                          table(D, B) if tab is None else tab, own)
    return hit.reshape(Q, WMAX - 1, hop)


def programme(cost, hit, n_wp, hop=HOP):
    """Per query shortcut_model.dp on reserve_poly_model.admit(cost, hit) (hit None: on cost), and chain_hit."""
    out = []
    for k in range(len(n_wp)):
        W = XM.w_of(n_wp, k)
        c = cost[k] if hit is None else RPM.admit(cost[k], hit[k])
        out.append(XM.dp(c, W, hop) + ((RPM.chain_hit(hit[k], W) if hit is not None else None),))
    return out


@functools.lru_cache(maxsize=None)
def reference(D, control, B):
    b = XM.batch(D, control)
    t_rows = b["states"][4 * D + 1]
    t0, radius, ignore = query_rows(D, B)
    _, cost, _ = dense(D, control)
    hit = hits(D, control, B, pair_rows(t_rows, t0, radius, ignore, HOP))
    return {"cost": cost, "hit": hit, "untimed": programme(cost, None, b["n_wp"]), "timed": programme(cost, hit, b["n_wp"])}


def counts(D, control, B):
    """The conditions of tests/test_shortcut_timed_cases.py, as numbers."""
    b = XM.batch(D, control)
    n_wp, t_rows = b["n_wp"], b["states"][4 * D + 1]
    t0, radius, ignore = query_rows(D, B)
    ref = reference(D, control, B)
    cost, hit = ref["cost"], ref["hit"]
    dp = dense(D, control)[0]
    solved = (dp.status == 0).reshape(hit.shape)
    admitted = np.isfinite(cost) & solved
    admitted[:, :, 0] = False
    live = [k for k in range(Q) if ref["untimed"][k][0] == 0]
    ch = np.array([ref["timed"][k][4] for k in live])
    adj = hit[:, :, 0]
    both = sum(1 for k in live if (adj[k, :XM.w_of(n_wp, k) - 1] == -2).any() and (adj[k, :XM.w_of(n_wp, k) - 1] >= 0).any())
    same0 = hits(D, control, B, pair_rows(t_rows, np.full(Q, t0[0]), np.full(Q, radius[0]), np.full(Q, ignore[0], np.int32), HOP))
    padded = np.full((WMAX, PAD_STRIDE), np.nan)
    padded[:, :Q] = t_rows
    flat = padded.ravel()
    wrong = hits(D, control, B, pair_rows(t_rows, t0, radius, ignore, HOP, t_at=lambda i, k: flat[i * Q + k]))
    nobody = hits(D, control, B, pair_rows(t_rows, t0, radius, np.full(Q, -1, np.int32), HOP))
    n_solved = int(solved.sum())
    return {"admitted": int(admitted.sum()), "blocked": int((admitted & (hit != -1)).sum()),
            "blocked_horizon": int((admitted & (hit == -2)).sum()), "live": len(live),
            "keep_changes": sum(1 for k in live if ref["timed"][k][1] != ref["untimed"][k][1]),
            "chain_hit": int((ch >= 0).sum()), "chain_horizon": int((ch == -2).sum()), "chain_clear": int((ch == -1).sum()),
            "both_on_chain": both, "solved": n_solved, "query0_changes": int((solved & (same0 != hit)).sum()),
            "stride_changes": int((solved & (wrong != hit)).sum()), "ignore_changes": int((solved & (nobody != hit)).sum()),
            "partner_256": int(((hit >= 0) & ((hit & 0xffffffff) >= 256)).sum())}
