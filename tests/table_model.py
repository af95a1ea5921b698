"""A plain sequential restatement of include/mplx_table.h (the loop of reference graph_search.h:79-143 over the counting
entries of a batch of successor lists, in ascending entry index), a sweep built on it, and a heap Dijkstra over the same
successor provider.  Test infrastructure: dicts and Python floats, nothing shared with the engine.

Lists are dicts in the mplx_succ_lists layout: "stride" S, "count" [n], "action" / "cost" / "hash" [n * S], "state"
[4D+2][n * S].  A provider maps states [4D+2][n] to such lists.
"""
import heapq
import math

import numpy as np


def lists_from_oracle(O, oenv, states):
    """The oracle's dense slots of `states` as lists with stride nU (blocked successors included with cost +inf)."""
    states = np.ascontiguousarray(states, dtype=np.float64)
    n, nU = states.shape[1], oenv.U.shape[0]
    d = O.expand(oenv, states)
    st = d["status"].reshape(n, nU)
    emit = (st == 1) | (st == 2)
    rank = np.cumsum(emit, axis=1) - 1
    src = np.nonzero(emit.ravel())[0]
    dst = (src // nU) * nU + rank.ravel()[src]
    out = {"stride": nU, "count": emit.sum(axis=1).astype(np.int32), "action": np.zeros(n * nU, np.int32),
           "cost": np.zeros(n * nU, np.float64), "hash": np.zeros(n * nU, np.uint64),
           "state": np.zeros((states.shape[0], n * nU), np.float64)}
    out["action"][dst] = (src % nU).astype(np.int32)
    out["cost"][dst] = d["cost"][src]
    out["hash"][dst] = d["hash"][src]
    out["state"][:, dst] = d["state"][:, src]
    return out


def oracle_provider(O, oenv):
    return lambda states: lists_from_oracle(O, oenv, states)


class TableModel:
    def __init__(self, n_fields):
        self.n_fields = n_fields
        self.ids = {}  # hash -> node id
        self.hash, self.g, self.pred, self.pred_action, self.state = [], [], [], [], []
        self.counting = 0  # counting entries seen so far

    @property
    def n_nodes(self):
        return len(self.hash)

    def arrays(self):
        st = np.array(self.state, dtype=np.float64).reshape(self.n_nodes, self.n_fields).T
        return {"n_nodes": self.n_nodes, "hash": np.array(self.hash, dtype=np.uint64), "g": np.array(self.g, dtype=np.float64),
                "pred": np.array(self.pred, dtype=np.int32), "pred_action": np.array(self.pred_action, dtype=np.int32),
                "state": np.ascontiguousarray(st)}

    def _walk(self, entries, n_entries):
        """entries: (e, hash, cand, pred, action, state column) in ascending e.  Returns (frontier, entry_id)."""
        entry_id = np.full(n_entries, -1, np.int32)
        winner = {}  # node id -> the entry that set its g last
        for e, h, cand, pred, action, col in entries:
            self.counting += 1
            i = self.ids.get(h)
            if i is None:  # graph_search.h:87-97: a new state, g = +inf
                i = self.n_nodes
                self.ids[h] = i
                self.hash.append(h)
                self.g.append(math.inf)
                self.pred.append(-1)
                self.pred_action.append(-1)
                self.state.append(np.array(col, dtype=np.float64))
            entry_id[e] = i
            if cand < self.g[i]:  # graph_search.h:107-109
                self.g[i] = cand
                self.pred[i] = pred
                self.pred_action[i] = action
                winner[i] = e
        order = sorted(winner, key=lambda i: winner[i])
        st = np.zeros((self.n_fields, len(order)))
        for r, i in enumerate(order):
            st[:, r] = self.state[i]
        return {"count": len(order), "id": np.array(order, dtype=np.int32), "g": np.array([self.g[i] for i in order], dtype=np.float64),
                "state": st}, entry_id

    def seed(self, states, hashes, g=None):
        states = np.asarray(states, dtype=np.float64).reshape(self.n_fields, -1)
        n = states.shape[1]
        gs = np.zeros(n) if g is None else np.broadcast_to(np.asarray(g, dtype=np.float64), (n,))

        def entries():
            for e in range(n):
                cand = float(gs[e])
                if math.isfinite(cand) and cand >= 0.0:
                    yield e, int(hashes[e]), cand + 0.0, -1, -1, states[:, e]
        return self._walk(entries(), n)

    def relax(self, lists, parent_id, parent_g, g_max=math.inf, n_nodes=None):
        S = int(lists["stride"])
        n = len(lists["count"]) if n_nodes is None else int(n_nodes)
        count, action, cost, hsh, state = lists["count"], lists["action"], lists["cost"], lists["hash"], lists["state"]

        def entries():
            for k in range(n):
                if parent_id[k] < 0:
                    continue
                pg = np.float64(parent_g[k])
                for j in range(int(count[k])):
                    e = k * S + j
                    c = np.float64(cost[e])
                    if not np.isfinite(c):
                        continue
                    cand = pg + c  # one IEEE add
                    if not (np.isfinite(cand) and cand >= 0.0 and cand <= g_max):
                        continue
                    yield e, int(hsh[e]), float(cand) + 0.0, int(parent_id[k]), int(action[e]), state[:, e]
        return self._walk(entries(), n * S)


def sweep(model, provider, starts, hashes, g=None, g_max=math.inf, max_rounds=None, on_round=None):
    """seed; then while the frontier is not empty: lists of the frontier's states, relax.  Returns the number of relax
    calls and the largest frontier.  on_round(round, lists, frontier_in, frontier_out, entry_id) sees every round."""
    fr, _ = model.seed(starts, hashes, g)
    rounds, largest = 0, fr["count"]
    while fr["count"] > 0 and (max_rounds is None or rounds < max_rounds):
        lists = provider(fr["state"])
        nxt, entry_id = model.relax(lists, fr["id"], fr["g"], g_max)
        rounds += 1
        if on_round:
            on_round(rounds, lists, fr, nxt, entry_id)
        fr = nxt
        largest = max(largest, fr["count"])
    return rounds, largest


def dijkstra(provider, start, start_hash, g_max=math.inf):
    """Heap Dijkstra over the provider's successors, one node per pop: {hash: g} of every state with g <= g_max."""
    start = np.asarray(start, dtype=np.float64).reshape(-1)
    g = {int(start_hash): 0.0}
    state = {int(start_hash): start}
    done = set()
    heap = [(0.0, int(start_hash))]
    while heap:
        gu, hu = heapq.heappop(heap)
        if hu in done or gu > g[hu]:
            continue
        done.add(hu)
        lists = provider(state[hu].reshape(-1, 1))
        for j in range(int(lists["count"][0])):
            c = np.float64(lists["cost"][j])
            if not np.isfinite(c):
                continue
            cand = float(np.float64(gu) + c)
            if not cand <= g_max:
                continue
            hv = int(lists["hash"][j])
            if cand < g.get(hv, math.inf):
                g[hv] = cand
                if hv not in state:
                    state[hv] = lists["state"][:, j].copy()
                heapq.heappush(heap, (cand, hv))
    return g
