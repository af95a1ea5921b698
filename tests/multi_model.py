"""A plain sequential restatement of include/mplx_multi.h over tests/table_model.py and tests/open_model.py: a node table
whose nodes are (query, hash) pairs, an open set with one goal per query, select_many and the loop of EnvMap.search_many.
Test infrastructure: dicts and Python floats, nothing shared with the engine.

restrict() is the renumbering under which query q of a batch must equal the single-query objects bit for bit: the nodes
of q in id order, their ids replaced by their ranks, pred taken through the same map.
"""
import math

import numpy as np

import open_model as OM
from table_model import TableModel

IS_OPEN, IS_GOAL, SEEN = OM.IS_OPEN, OM.IS_GOAL, OM.SEEN
SELECTED, FOUND, EMPTY, MAX_ROUNDS, MAX_EXPAND = OM.SELECTED, OM.FOUND, OM.EMPTY, OM.MAX_ROUNDS, OM.MAX_EXPAND


class MultiTableModel(TableModel):
    """TableModel keyed by (query, hash).  `query` is the per-node column."""

    def __init__(self, n_fields, n_queries):
        super().__init__(n_fields)
        self.n_queries = int(n_queries)
        self.query = []

    def arrays(self):
        a = super().arrays()
        a["query"] = np.array(self.query, dtype=np.int32)
        return a

    def _walk_keyed(self, entries, n_entries):
        """entries as TableModel._walk takes them, with (query, hash) in the place of the hash."""
        before = self.n_nodes
        out = super()._walk(entries, n_entries)
        for i in range(before, self.n_nodes):  # the base class stored the key where the hash goes
            q, h = self.hash[i]
            self.hash[i] = h
            self.query.append(q)
        return out

    def seed(self, states, hashes, g=None, query=None):
        states = np.asarray(states, dtype=np.float64).reshape(self.n_fields, -1)
        n = states.shape[1]
        gs = np.zeros(n) if g is None else np.broadcast_to(np.asarray(g, dtype=np.float64), (n,))
        qs = np.zeros(n, np.int64) if query is None else np.broadcast_to(np.asarray(query), (n,))
        assert all(0 <= int(q) < self.n_queries for q in qs)  # (MPLX_ERR_ARG on the device)

        def entries():
            for e in range(n):
                cand = float(gs[e])
                if math.isfinite(cand) and cand >= 0.0:
                    yield e, (int(qs[e]), int(hashes[e])), cand + 0.0, -1, -1, states[:, e]
        return self._walk_keyed(entries(), n)

    def relax(self, lists, parent_id, parent_g, g_max=math.inf, n_nodes=None):
        S = int(lists["stride"])
        n = len(lists["count"]) if n_nodes is None else int(n_nodes)
        count, action, cost, hsh, state = lists["count"], lists["action"], lists["cost"], lists["hash"], lists["state"]
        n_before = self.n_nodes

        def entries():
            for k in range(n):
                p = int(parent_id[k])
                if p < 0 or p >= n_before:  # not a node that existed before the call: the row does not count
                    continue
                q = self.query[p]
                pg = np.float64(parent_g[k])
                for j in range(int(count[k])):
                    e = k * S + j
                    c = np.float64(cost[e])
                    if not np.isfinite(c):
                        continue
                    cand = pg + c  # one IEEE add
                    if not (np.isfinite(cand) and cand >= 0.0 and cand <= g_max):
                        continue
                    yield e, (q, int(hsh[e])), float(cand) + 0.0, p, int(action[e]), state[:, e]
        return self._walk_keyed(entries(), n * S)

    def find(self, hashes, query):
        return np.array([self.ids.get((int(q), int(h)), -1) for h, q in zip(hashes, query)], dtype=np.int32)


class MultiOpenModel(OM.OpenModel):
    """OpenModel with goals[query of the node]: goal_rows [Q][4D+2], goal_hashes [Q], blocked: None or one callable per
    query (the ray trace towards that query's goal)."""

    def __init__(self, table, dim, goal_rows, goal_hashes, w, v_max, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0, tol_yaw=-1.0,
                 blocked=None):
        super().__init__(table, dim, goal_rows[0], goal_hashes[0], w, v_max, tol_pos, tol_vel, tol_acc, tol_yaw)
        self.goals = [[float(x) for x in np.asarray(r, dtype=np.float64)] for r in goal_rows]
        self.goal_hashes = [int(h) for h in goal_hashes]
        self.blocked_q = blocked
        assert len(self.goals) == len(self.goal_hashes) == table.n_queries

    def heur_and_tol(self, node_id, s):
        q = self.table.query[node_id]
        self.goal, self.goal_hash = self.goals[q], self.goal_hashes[q]
        return super().heur_and_tol(node_id, s)

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
        for r, i, ok in rows:
            hit = False
            if ok and sight:
                hit = bool(self.blocked_q[self.table.query[i]](np.asarray(fr["state"])[:self.dim, [r]].T)[0])
            self.flags[i] = SEEN | IS_OPEN | (IS_GOAL if ok and not hit else 0)

    def select(self, delta, capacity):
        raise TypeError("an open set of several queries: select_many")

    def select_many(self, delta, capacity):
        """(results [Q], frontier): the rule of OpenModel.select per query, the union in id order cut at `capacity`."""
        Q = self.table.n_queries
        res, marked = [], []
        Os, Gs = [[] for _ in range(Q)], [[] for _ in range(Q)]
        for i in sorted(self.flags):
            if self.flags[i] & IS_OPEN:
                Os[self.table.query[i]].append(i)
            if self.flags[i] & IS_GOAL:
                Gs[self.table.query[i]].append(i)
        for q in range(Q):
            O, G = Os[q], Gs[q]
            f_min = min([self.f[i] for i in O], default=math.inf)
            goal_f = min([self.f[i] for i in G], default=math.inf)
            goal_id = min([i for i in G if self.f[i] == goal_f], default=-1)
            goal_g = float(self.table.g[goal_id]) if goal_id >= 0 else math.inf
            if G and goal_f <= f_min:
                status = FOUND
            elif not O:
                status = EMPTY
            else:
                status = SELECTED
                T = f_min + float(delta)
                marked += [i for i in O if self.f[i] <= T]
            res.append({"status": status, "goal_id": goal_id, "count": 0, "n_open": len(O), "f_min": f_min, "goal_f": goal_f,
                        "goal_g": goal_g})
        chosen = sorted(marked)[:int(capacity)]
        for i in chosen:
            self.flags[i] &= ~IS_OPEN
            r = res[self.table.query[i]]
            r["count"] += 1
            r["n_open"] -= 1
        st = np.zeros((self.table.n_fields, len(chosen)))
        for r, i in enumerate(chosen):
            st[:, r] = self.table.state[i]
        fr = {"count": len(chosen), "id": np.array(chosen, dtype=np.int32),
              "g": np.array([self.table.g[i] for i in chosen], dtype=np.float64), "state": st}
        return res, fr


def search_many(table, opn, provider, starts, start_hashes, eps, delta, capacity, g_max=math.inf, sight=0, max_rounds=None,
                max_expand=None, on_round=None):
    """The loop of EnvMap.search_many on the model.  Returns a dict: status [Q], results (the last select's), rounds [Q]
    (rounds in which the query selected), expanded [Q], total_rounds, history [Q] (the result of every round in which the
    query selected), truncated (selections cut at `capacity`).  on_round(round, results, sel, lists, imp) sees every
    round."""
    Q = table.n_queries
    imp, _ = table.seed(starts, start_hashes, query=np.arange(Q))
    opn.push(imp, imp["count"], eps, sight)
    total = truncated = 0
    rounds, expanded, history = [0] * Q, [0] * Q, [[] for _ in range(Q)]
    limit = None
    while True:
        res, sel = opn.select_many(delta, capacity)
        if not any(r["status"] == SELECTED for r in res):
            break
        if max_rounds is not None and total >= max_rounds:
            limit = MAX_ROUNDS
        elif max_expand is not None and sum(expanded) + sel["count"] > max_expand:
            limit = MAX_EXPAND
        if limit is not None:
            opn.push(sel, sel["count"], eps, sight)
            break
        if sel["count"] == capacity:
            truncated += any(fl & IS_OPEN and res[table.query[i]]["status"] == SELECTED and
                             opn.f[i] <= res[table.query[i]]["f_min"] + delta for i, fl in opn.flags.items())
        lists = provider(sel["state"])
        imp, _ = table.relax(lists, sel["id"], sel["g"], g_max)
        opn.push(imp, sel["count"] * int(lists["stride"]), eps, sight)
        total += 1
        for q, r in enumerate(res):
            if r["status"] == SELECTED:
                rounds[q] += 1
                expanded[q] += r["count"]
                history[q].append(dict(r))
        if on_round:
            on_round(total, res, sel, lists, imp)
    status = [limit if (r["status"] == SELECTED and limit is not None) else r["status"] for r in res]
    return {"status": status, "results": res, "rounds": rounds, "expanded": expanded, "total_rounds": total, "history": history,
            "truncated": truncated}


def restrict(tab, q, f=None, flags=None):
    """Query q of a batch under the renumbering: tab = the arrays of a table with "query" (the model's arrays() or the
    device's download()); f / flags: the open set's arrays.  Returns (table arrays of q with pred renumbered, f, flags,
    rank): rank[global id] = the id inside q, -1 for other queries' nodes."""
    query = np.asarray(tab["query"])
    mine = np.nonzero(query == q)[0]
    rank = np.full(query.size, -1, np.int64)
    rank[mine] = np.arange(mine.size)
    pred = np.asarray(tab["pred"])[mine].astype(np.int64)
    assert np.all(query[pred[pred >= 0]] == q)  # a node's best parent is a node of its own query
    out = {"n_nodes": int(mine.size), "hash": np.asarray(tab["hash"])[mine], "g": np.asarray(tab["g"])[mine],
           "pred": np.where(pred >= 0, rank[np.maximum(pred, 0)], -1).astype(np.int32),
           "pred_action": np.asarray(tab["pred_action"])[mine], "state": np.asarray(tab["state"])[:, mine]}
    return out, (None if f is None else np.asarray(f)[mine]), (None if flags is None else np.asarray(flags)[mine]), rank


def renumber_result(res, rank):
    """A query's result with goal_id taken through the renumbering."""
    out = dict(res)
    out["goal_id"] = int(rank[res["goal_id"]]) if res["goal_id"] >= 0 else -1
    return out


# ---- the hand-built scenario of tests/test_gpu_multi.py (tests/test_multi.py runs it through the models on the CPU)
HAND_Q, HAND_W, HAND_VMAX, HAND_TOL = 3, 10.0, 1.0, 0.25
HAND_GOALS = ((0.2, 0.1), (0.2, 0.1), (0.6, 0.3))  # queries 0 and 1 share their goal


def hand_seeds(seed=7):
    """40 distinct 2D ACC states at rest on a lattice of 0.1 m; states 0 .. 29 are seeded into query s % 3, states
    0 .. 11 into query (s + 1) % 3 as well (the same hash in two queries: two nodes), three of them twice into the same
    query (one node), in shuffled order; g from three values, + 100 inside the query's goal region.  Returns (states [10][n], query [n], g [n], goal_rows [3][10])."""
    from table_model import F2
    rng = np.random.default_rng(seed)
    ix, iy = np.meshgrid(np.arange(8), np.arange(5))
    order = rng.permutation(40)
    pos = np.stack([ix.ravel() * 0.1, iy.ravel() * 0.1])[:, order]
    pairs = [(s, s % 3) for s in range(30)] + [(s, (s + 1) % 3) for s in range(12)] + [(s, s % 3) for s in (3, 4, 5)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    states = np.zeros((F2, len(pairs)))
    states[:2] = pos[:, [s for s, _ in pairs]]
    query = np.array([q for _, q in pairs], dtype=np.int32)
    goals = np.zeros((HAND_Q, F2))
    goals[:, :2] = HAND_GOALS
    # the goal regions are dear (g + 100), so the first selects are SELECTED and the goal is announced late
    near = np.abs(states[:2] - goals[query, :2].T).max(axis=0) <= HAND_TOL
    g = rng.choice([0.0, 0.5, 1.0], size=len(pairs)) + np.where(near, 100.0, 0.0)
    return states, query, g, goals


def hand_relax(rng, n_before, n=60, S=8):
    """Crafted lists against a table of n_before nodes: a small pool of hashes (the same hash turns up under parents of
    different queries, equal candidates inside one query are common) with the hash equal to the empty marker in it;
    parents drawn from the nodes, and rows whose parent is no node of the table: -1, n_before, n_before + 5, 2^31 - 1."""
    from table_model import EMPTY, hand_lists
    pool = np.concatenate([rng.integers(1, 2 ** 63, size=30, dtype=np.uint64), np.full(4, EMPTY, np.uint64)])
    lists = hand_lists(rng, n, S, pool, poison_base=0xBEEF00000000, inf_rate=0.05, nan_rate=0.05)
    parent_id = rng.integers(0, n_before, size=n).astype(np.int32)
    parent_id[[5, 11, 17, 23]] = [-1, n_before, n_before + 5, 2 ** 31 - 1]
    parent_g = rng.choice([0.0, 0.5, 1.0, 1.5], size=n)
    return lists, parent_id, parent_g, pool


def split_rows(lists, parent_id, parent_g, row_query, rank, q):
    """The rows of a batch relax that belong to query q (row_query[k] == q), in order, with the parents renumbered."""
    S = int(lists["stride"])
    rows = np.nonzero(np.asarray(row_query) == q)[0]
    ent = (rows[:, None] * S + np.arange(S)[None, :]).ravel()
    sub = {"stride": S, "count": np.asarray(lists["count"])[rows], "action": np.asarray(lists["action"])[ent],
           "cost": np.asarray(lists["cost"])[ent], "hash": np.asarray(lists["hash"])[ent], "state": np.asarray(lists["state"])[:, ent]}
    return sub, rank[np.asarray(parent_id)[rows]].astype(np.int32), np.asarray(parent_g)[rows]
