"""The model mplx_shortcut (include/mplx_limits.h) is compared with: the dynamic programme over the hops of one chain, a
brute force over every chain of hops, and the edge costs of a pair set from the coefficients the device returned.

Costs of a chain of W states: c[i][h] is the cost of the hop i -> i + h + 1 (h < max_hop), +inf where the hop is not
admitted, NaN on an adjacent hop whose solve failed (a bad chain).  dist[0] = 0.0, dist[j] = min over max(0, j - max_hop)
<= i < j of dist[i] + c[i][j - i - 1], one add per candidate, ties to the smallest i."""
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


def edge_costs(pairs, max_hop, D, so, control, w, limits, world):
    """c of every pair from what the device holds in `pairs` (coefficients, yaw, dts, status): [P], pair p = (k (w_max - 1)
    + i) max_hop + (j - i - 1).  limits = (v_max,
    a_max, j_max); world = (grid, pot or None, md, org, res, v_max, pot_w, grad_w) of traj_model.traverse."""
    coef, yaw, dts, status = pairs.coefficients(), pairs.yaw_coefficients(), pairs.dts(), pairs.status
    P = pairs.n
    out = np.zeros(P)
    for p in range(P):
        adjacent = p % max_hop == 0
        if status[p]:
            out[p] = np.nan if adjacent else np.inf
            continue
        tr = SM.PolySet(coef[:1, :, :, p].reshape(-1, D), yaw[:1, :, p].reshape(-1), dts[:1, p], so, D)
        trav = F(TM.traverse(tr, *world)["cost"])
        base = tr.effort[so] + F(w) * F(tr.T)
        if adjacent:
            out[p] = base + (trav if np.isfinite(trav) else F(0.0))
        else:
            valid = LM.traj_limits([tr.coef[0]], tr.dts, control, *limits, LM.ALL_ROOTS)["valid"]
            out[p] = base + trav if (valid == 1 and np.isfinite(trav)) else np.inf
    return out
