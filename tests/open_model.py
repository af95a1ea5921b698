"""A plain sequential restatement of include/mplx_open.h over tests/table_model.py::TableModel: keys and flags per node,
push, select, and the search loop of EnvMap.search built on them.  Test infrastructure: Python floats (IEEE doubles, no
contraction) and dicts, nothing shared with the engine.  OpenArrays restates push and select once more on whole numpy arrays, for
tables the loops cannot follow (tests/large_case.py); tests/test_open.py pins it to OpenModel bit for bit.

Frontiers are the dicts TableModel emits ("count", "id", "g", "state" [4D+2][count]).  `blocked(positions [n][D])` is the
ray trace of env_map::is_goal (True: an occupied cell on the ray to the goal); ray_blocked() builds it from
tests/ray_model.py.
"""
import math

import numpy as np

IS_OPEN, IS_GOAL, SEEN = 1, 2, 4
SELECTED, FOUND, EMPTY = 0, 1, 2
MAX_ROUNDS, MAX_EXPAND = 3, 4


def ray_blocked(grid, map_dim, origin, res, goal_pos):
    from ray_model import HIT, ray_trace

    def blocked(p1):
        p1 = np.ascontiguousarray(p1, dtype=np.float64)
        m = ray_trace(np.asarray(grid).ravel(), map_dim, origin, res, p1, np.broadcast_to(np.asarray(goal_pos, dtype=np.float64), p1.shape))
        return (m["status"] & HIT) > 0
    return blocked


class OpenModel:
    def __init__(self, table, dim, goal_row, goal_hash, w, v_max, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0, tol_yaw=-1.0, blocked=None):
        self.table, self.dim = table, dim
        self.goal = [float(x) for x in np.asarray(goal_row, dtype=np.float64)]
        self.goal_hash = int(goal_hash)
        self.w, self.v_max = float(w), float(v_max)
        self.tol = (float(tol_pos), float(tol_vel), float(tol_acc), float(tol_yaw))
        self.blocked = blocked
        self.f, self.flags = {}, {}  # node id -> key / flags byte

    def heur_and_tol(self, node_id, s):
        """env_base.h:46-64 (default branch) and env_map.h:25-37 without the ray trace, for state column s."""
        D, g = self.dim, self.goal
        linf = lambda a, b: max([0.0] + [abs(float(s[a + i]) - g[b + i]) for i in range(D)])
        m = linf(0, 0)
        if int(self.table.hash[node_id]) == self.goal_hash:
            h = 0.0
        else:
            h = self.w * m / self.v_max if self.v_max > 0 else self.w * m
        tol_pos, tol_vel, tol_acc, tol_yaw = self.tol
        ok = m <= tol_pos
        if ok and tol_vel >= 0:
            ok = linf(D, D) <= tol_vel
        if ok and tol_acc >= 0:
            ok = linf(2 * D, 2 * D) <= tol_acc
        if ok and tol_yaw >= 0:
            ok = abs(float(s[4 * D]) - g[4 * D]) <= tol_yaw
        return h, ok

    def push(self, fr, n_max, eps, sight=0, capacity=None):
        n = min(int(fr["count"]), int(n_max))
        if capacity is not None:
            n = min(n, int(capacity))
        rows = []
        for r in range(n):
            i = int(fr["id"][r])
            if not 0 <= i < self.table.n_nodes:
                continue
            h, ok = self.heur_and_tol(i, fr["state"][:, r])
            g = float(fr["g"][r])
            f = g if eps == 0 else g + float(eps) * h
            if not f >= 0.0:
                continue
            self.f[i] = f + 0.0
            rows.append((r, i, ok))
        cand = [r for r, i, ok in rows if ok]
        hit = {}
        if sight and cand:
            if self.blocked is None:
                raise ValueError("sight needs blocked()")
            b = self.blocked(np.asarray(fr["state"])[:self.dim, cand].T)
            hit = {r: bool(x) for r, x in zip(cand, b)}
        for r, i, ok in rows:
            self.flags[i] = SEEN | IS_OPEN | (IS_GOAL if ok and not hit.get(r, False) else 0)

    def arrays(self):
        """f and flags as the device holds them for nodes [0, n_nodes); f is compared only where SEEN is set."""
        n = self.table.n_nodes
        f, fl = np.zeros(n), np.zeros(n, np.uint8)
        for i, v in self.f.items():
            f[i] = v
        for i, v in self.flags.items():
            fl[i] = v
        return f, fl

    def select(self, delta, capacity):
        O = sorted(i for i, fl in self.flags.items() if fl & IS_OPEN)
        G = sorted(i for i, fl in self.flags.items() if fl & IS_GOAL)
        f_min = min([self.f[i] for i in O], default=math.inf)
        goal_f = min([self.f[i] for i in G], default=math.inf)
        goal_id = min([i for i in G if self.f[i] == goal_f], default=-1)
        goal_g = float(self.table.g[goal_id]) if goal_id >= 0 else math.inf
        chosen = []
        if G and goal_f <= f_min:
            status = FOUND
        elif not O:
            status = EMPTY
        else:
            status = SELECTED
            T = f_min + float(delta)
            chosen = [i for i in O if self.f[i] <= T][:int(capacity)]
            for i in chosen:
                self.flags[i] &= ~IS_OPEN
        st = np.zeros((self.table.n_fields, len(chosen)))
        for r, i in enumerate(chosen):
            st[:, r] = self.table.state[i]
        fr = {"count": len(chosen), "id": np.array(chosen, dtype=np.int32),
              "g": np.array([self.table.g[i] for i in chosen], dtype=np.float64), "state": st}
        res = {"status": status, "goal_id": goal_id, "count": len(chosen), "n_open": len(O) - len(chosen), "f_min": f_min,
               "goal_f": goal_f, "goal_g": goal_g}
        return res, fr


class OpenArrays:
    """OpenModel's push and select on whole arrays (no ray trace): the same IEEE operations in the same order, the same
    return values.  `table`: anything with n_nodes, n_fields, hash, g [n_nodes] and state [n_fields][n_nodes] as arrays
    (tests/table_model.py::TableArrays); it may grow between calls."""

    def __init__(self, table, dim, goal_row, goal_hash, w, v_max, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0, tol_yaw=-1.0):
        self.table, self.dim = table, dim
        self.goal = np.asarray(goal_row, dtype=np.float64)
        self.goal_hash = np.uint64(goal_hash)
        self.w, self.v_max = float(w), float(v_max)
        self.tol = (float(tol_pos), float(tol_vel), float(tol_acc), float(tol_yaw))
        self.f, self.flags = np.zeros(0), np.zeros(0, np.uint8)

    def _grow(self):
        more = self.table.n_nodes - self.f.size
        if more > 0:
            self.f, self.flags = np.concatenate([self.f, np.zeros(more)]), np.concatenate([self.flags, np.zeros(more, np.uint8)])

    def heur_and_tol(self, ids, s):
        """OpenModel.heur_and_tol for the state columns s of nodes ids."""
        D, g = self.dim, self.goal
        # (max() over Python floats starts at 0.0 and never takes a NaN: fmax)
        linf = lambda a, b: np.fmax.reduce(np.abs(s[a:a + D] - g[b:b + D, None]), axis=0, initial=0.0)
        m = linf(0, 0)
        h = self.w * m / self.v_max if self.v_max > 0 else self.w * m
        h = np.where(np.asarray(self.table.hash)[ids] == self.goal_hash, 0.0, h)
        tol_pos, tol_vel, tol_acc, tol_yaw = self.tol
        ok = m <= tol_pos
        if tol_vel >= 0:
            ok &= linf(D, D) <= tol_vel
        if tol_acc >= 0:
            ok &= linf(2 * D, 2 * D) <= tol_acc
        if tol_yaw >= 0:
            ok &= np.abs(s[4 * D] - g[4 * D]) <= tol_yaw
        return h, ok

    def push(self, fr, n_max, eps, capacity=None):
        self._grow()
        n = min(int(fr["count"]), int(n_max))
        if capacity is not None:
            n = min(n, int(capacity))
        ids = np.asarray(fr["id"][:n]).astype(np.int64)
        inside = (ids >= 0) & (ids < self.table.n_nodes)
        ids, g, s = ids[inside], np.asarray(fr["g"][:n], dtype=np.float64)[inside], np.asarray(fr["state"])[:, :n][:, inside]
        h, ok = self.heur_and_tol(ids, s)
        with np.errstate(invalid="ignore"):
            f = g if eps == 0 else g + float(eps) * h
            keep = f >= 0.0
        ids, f, ok = ids[keep], f[keep], ok[keep]
        self.f[ids] = f + 0.0
        self.flags[ids] = (SEEN | IS_OPEN) | np.where(ok, IS_GOAL, 0).astype(np.uint8)

    def arrays(self):
        self._grow()
        return self.f, self.flags

    def select(self, delta, capacity):
        self._grow()
        t = self.table
        O, G = np.nonzero(self.flags & IS_OPEN)[0], np.nonzero(self.flags & IS_GOAL)[0]
        f_min = float(self.f[O].min()) if O.size else math.inf
        goal_f = float(self.f[G].min()) if G.size else math.inf
        goal_id = int(G[self.f[G] == goal_f][0]) if G.size else -1
        goal_g = float(t.g[goal_id]) if goal_id >= 0 else math.inf
        chosen = np.zeros(0, np.int64)
        if G.size and goal_f <= f_min:
            status = FOUND
        elif not O.size:
            status = EMPTY
        else:
            status = SELECTED
            T = f_min + float(delta)
            chosen = O[self.f[O] <= T][:int(capacity)]
            self.flags[chosen] &= np.uint8(0xff & ~IS_OPEN)
        fr = {"count": chosen.size, "id": chosen.astype(np.int32), "g": np.asarray(t.g)[chosen], "state": np.asarray(t.state)[:, chosen]}
        res = {"status": status, "goal_id": goal_id, "count": int(chosen.size), "n_open": int(O.size - chosen.size), "f_min": f_min,
               "goal_f": goal_f, "goal_g": goal_g}
        return res, fr


def search(table, opn, provider, start, start_hash, eps, delta, capacity, g_max=math.inf, sight=0, max_rounds=None,
           max_expand=None, on_round=None):
    """The loop of EnvMap.search on the model.  Returns a dict: status, result (the last select's), rounds (relax calls),
    expanded, truncated (selections cut at `capacity`).  on_round(round, sel, lists, imp) sees every round."""
    imp, _ = table.seed(start, [start_hash])
    opn.push(imp, imp["count"], eps, sight)
    rounds = expanded = truncated = 0
    while True:
        before = sum(1 for fl in opn.flags.values() if fl & IS_OPEN)
        res, sel = opn.select(delta, capacity)
        status = res["status"]
        if status != SELECTED:
            break
        if max_rounds is not None and rounds >= max_rounds:
            status = MAX_ROUNDS
        elif max_expand is not None and expanded + sel["count"] > max_expand:
            status = MAX_EXPAND
        if status != SELECTED:
            opn.push(sel, sel["count"], eps, sight)
            break
        if sel["count"] == capacity and res["n_open"] > 0:
            T = res["f_min"] + delta
            truncated += any(fl & IS_OPEN and opn.f[i] <= T for i, fl in opn.flags.items())
        lists = provider(sel["state"])
        imp, _ = table.relax(lists, sel["id"], sel["g"], g_max)
        opn.push(imp, sel["count"] * int(lists["stride"]), eps, sight)
        rounds += 1
        expanded += sel["count"]
        if on_round:
            on_round(rounds, sel, lists, imp)
    return {"status": status, "result": res, "rounds": rounds, "expanded": expanded, "truncated": truncated}


# ---- the hand-built scenario of tests/test_gpu_open.py (its properties are checked on the CPU by tests/test_open.py)
HAND_N, HAND_GOAL, HAND_W, HAND_VMAX, HAND_TOL = 5000, (3.0, 2.0), 10.0, 1.0, 0.5


def hand_scenario(seed=21):
    """5 000 distinct 2D ACC states on a 100 x 50 lattice of 0.1 m in shuffled order (ids span one full tile of 4 096
    and a partial one), a goal whose tolerance box holds 121 of them, and two pushes: `rows` (id, g) to process and
    `tail` rows behind them that no push may process (behind n_max in the first, behind the capacity in the second).
    g comes from 8 values, so equal keys are common.  Push 1 keeps the goal region dear (g + 100) and carries rows
    that must be ignored (ids outside the table, a NaN g, a key below zero); push 2 overlaps push 1 (closed nodes are
    re-opened, open keys replaced) and gives every goal-region node but the goal's own cell g = 50: the nodes at the
    same distance tie."""
    rng = np.random.default_rng(seed)
    ix, iy = np.meshgrid(np.arange(100), np.arange(50))
    order = rng.permutation(HAND_N)
    states = np.zeros((10, HAND_N))
    states[0] = (ix.ravel() * 0.1)[order]
    states[1] = (iy.ravel() * 0.1)[order]
    # (at rest: the lattice hash of waypoint.h collides for some position / velocity pairs, and the ids must be 5 000)
    goal = np.zeros(10)
    goal[:2] = HAND_GOAL
    linf = np.abs(states[:2] - goal[:2, None]).max(axis=0)
    in_goal, centre = linf <= HAND_TOL, linf == 0.0
    gvals = np.arange(8) * 0.5
    ids = np.arange(HAND_N)
    a = rng.choice(ids[~centre], 1500, replace=False)
    ga = rng.choice(gvals, a.size) + np.where(in_goal[a], 100.0, 0.0)
    ignored = rng.choice(np.setdiff1d(ids[~centre], a), 2, replace=False)
    bad_id = np.array([-1, HAND_N, 2 ** 31 - 1, ignored[0], ignored[1]])
    bad_g = np.array([0.0, 0.0, 0.0, np.nan, -1000.0])
    at = rng.choice(a.size, bad_id.size, replace=False)
    push1 = {"id": np.insert(a, at, bad_id), "g": np.insert(ga, at, bad_g)}
    rest = np.setdiff1d(ids[~centre], a)
    push1["tail_id"], push1["tail_g"] = rest[:50], np.zeros(50)
    b = np.union1d(rng.choice(ids[~centre], 1500, replace=False), ids[in_goal & ~centre])
    b = b[rng.permutation(b.size)]
    gb = np.where(in_goal[b], 50.0, rng.choice(gvals, b.size) + 1.0)
    push2 = {"id": b, "g": gb}
    rest2 = np.setdiff1d(rest, np.concatenate([b, ignored]))
    push2["tail_id"], push2["tail_g"] = rest2[:7], np.zeros(7)
    for p in (push1, push2):
        p["id"], p["tail_id"] = p["id"].astype(np.int64), p["tail_id"].astype(np.int64)
    return states, goal, in_goal, ignored, push1, push2


def hand_frontier(states, push, with_tail=False):
    """The frontier dict of a push's rows (rows with ids outside the table get zero states)."""
    ids = np.concatenate([push["id"], push["tail_id"]]) if with_tail else push["id"]
    g = np.concatenate([push["g"], push["tail_g"]]) if with_tail else push["g"]
    ok = (ids >= 0) & (ids < states.shape[1])
    st = np.zeros((states.shape[0], ids.size))
    st[:, ok] = states[:, ids[ok]]
    return {"count": ids.size, "id": ids.astype(np.int32), "g": g.astype(np.float64), "state": st}


# selects between the two pushes: (delta, capacity)
HAND_SELECTS = [(0.0, 0), (0.0, 16), (2.5, 16), (2.5, 5000), (math.inf, 16), (40.0, 5000)]
