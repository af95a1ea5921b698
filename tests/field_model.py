"""Sequential model of include/mplx_field.h: the goal distance field as a deque BFS over the stated neighbourhood, and
the push rule in float64, written in the header's order.  Pure numpy; no device, no library."""
import itertools
import math
from collections import deque

import numpy as np

INF_BITS = np.uint64(0x7FF0000000000000)


def float_to_int(x, origin, res):
    """MapUtil::floatToInt of one coordinate, (int)round((x - origin) / res - 0.5) with C's round (halves away from zero);
    None where the device's comparison as a double says "outside any map" (NaN, huge)."""
    v = (np.float64(x) - np.float64(origin)) / np.float64(res) - np.float64(0.5)
    if not np.isfinite(v) or abs(v) >= 2.0 ** 31:
        return None
    r = math.floor(v)
    d = v - r
    return int(r + 1 if (d >= 0.5 if v >= 0 else d > 0.5) else r)


def cell_of(pos, dims, origin, res):
    """The cell index (getIndex: x fastest) of a position, or None off the map."""
    idx, mul = 0, 1
    for i, n in enumerate(dims):
        c = float_to_int(pos[i], origin[i], res)
        if c is None or c < 0 or c >= n:
            return None
        idx += c * mul
        mul *= n
    return idx


def blocked_of(cells, region=None, potential=None):
    """Which cells are not traversable -- for the TESTS' maps only: occupied (100) or outside the region; with a potential
    map installed what ends a primitive there instead of the occupancy, a value >= 100 (env_map.h:113-118: values 1 .. 99
    cost, they do not block -- the context's own bits, a pre-screen, are set for them too, and the field does not use
    those bits then)."""
    cells = np.asarray(cells).ravel()
    b = (np.asarray(potential).ravel() >= 100) if potential is not None else (cells == 100)
    if region is not None:
        b = b | (np.asarray(region).ravel() == 0)
    return b


def field(blocked, dims, lo, hi):
    """dist [F][n_cells] int32.  blocked: bool [n_cells] (x fastest); dims: cells per axis (D of them); lo, hi: [F][D]
    inclusive seed boxes in cell indices."""
    dims = [int(d) for d in dims]
    D = len(dims)
    n = int(np.prod(dims))
    blocked = np.asarray(blocked, dtype=bool).ravel()
    assert blocked.size == n
    lo, hi = np.asarray(lo).reshape(-1, D), np.asarray(hi).reshape(-1, D)
    strides = [int(np.prod(dims[:i])) for i in range(D)]
    steps = [s for s in itertools.product((-1, 0, 1), repeat=D) if any(s)]
    out = np.full((lo.shape[0], n), -1, np.int32)
    for f in range(lo.shape[0]):
        a = [max(int(lo[f, i]), 0) for i in range(D)]
        b = [min(int(hi[f, i]), dims[i] - 1) for i in range(D)]
        if any(a[i] > b[i] for i in range(D)):
            continue
        dist = out[f]
        q = deque()
        for c in itertools.product(*[range(a[i], b[i] + 1) for i in reversed(range(D))]):
            c = c[::-1]
            idx = sum(c[i] * strides[i] for i in range(D))
            dist[idx] = 0
            q.append(c)
        while q:
            c = q.popleft()
            d = dist[sum(c[i] * strides[i] for i in range(D))]
            for s in steps:
                t = tuple(c[i] + s[i] for i in range(D))
                if any(t[i] < 0 or t[i] >= dims[i] for i in range(D)):
                    continue
                ti = sum(t[i] * strides[i] for i in range(D))
                if blocked[ti] or dist[ti] >= 0:
                    continue
                dist[ti] = d + 1
                q.append(t)
    return out


def chebyshev_to_box(dims, lo, hi):
    """[n_cells] Chebyshev distance of every cell to the (clipped) box: what dist would be on an empty map."""
    D = len(dims)
    grids = np.meshgrid(*[np.arange(dims[i]) for i in range(D)], indexing="ij")
    m = np.zeros(grids[0].shape, np.int64)
    for i in range(D):
        a, b = max(int(lo[i]), 0), min(int(hi[i]), dims[i] - 1)
        m = np.maximum(m, np.maximum(a - grids[i], 0) + np.maximum(grids[i] - b, 0))
    return np.transpose(m, list(reversed(range(D)))).ravel()  # x fastest


def goal_box(goal_pos, tol, origin, res):
    """GoalField.build's seed box: floatToInt(goal -+ tol) widened by one cell."""
    lo = [float_to_int(goal_pos[i] - tol, origin[i], res) - 1 for i in range(len(origin))]
    hi = [float_to_int(goal_pos[i] + tol, origin[i], res) + 1 for i in range(len(origin))]
    return lo, hi


def heuristic(pos, goal_pos, w, v_max, dist_f, dims, origin, res, is_goal_state=False):
    """(h, G, L) of one row of a query with a field (header section 4); G is None where the row has no finite grid distance."""
    pos, goal_pos = np.asarray(pos, np.float64), np.asarray(goal_pos, np.float64)
    L = np.float64(0)
    for i in range(len(dims)):
        d = abs(pos[i] - goal_pos[i])
        L = d if d > L else L
    if is_goal_state:
        return np.float64(0.0), None, L
    c = cell_of(pos, dims, origin, res)
    n = -1 if c is None else int(dist_f[c])
    if n < 0:
        return np.float64(np.inf), None, L
    G = np.float64(res) * np.float64(max(n - 1, 0))
    m = G if G > L else L
    h = np.float64(w) * m / np.float64(v_max) if v_max > 0 else np.float64(w) * m
    return h, G, L


def default_heuristic(pos, goal_pos, w, v_max, D, is_goal_state=False):
    """post_eval's heur: the key a push without a field uses."""
    L = np.float64(0)
    for i in range(D):
        d = abs(np.float64(pos[i]) - np.float64(goal_pos[i]))
        L = d if d > L else L
    if is_goal_state:
        return np.float64(0.0)
    return np.float64(w) * L / np.float64(v_max) if v_max > 0 else np.float64(w) * L


def key(g, eps, h):
    """f = g + eps * h (one multiply, one add; eps == 0: f = g), -0.0 -> +0.0; None for a row that is ignored."""
    f = np.float64(g)
    if eps != 0.0:
        with np.errstate(invalid="ignore"):
            f = np.float64(g) + np.float64(eps) * np.float64(h)
    if not f >= 0.0:
        return None
    return f + np.float64(0.0)
