"""A plain sequential restatement of include/mplx_table.h (the loop of reference graph_search.h:79-143 over the counting
entries of a batch of successor lists, in ascending entry index), a sweep built on it, and a heap Dijkstra over the same
successor provider.  Test infrastructure: dicts and Python floats, nothing shared with the engine.  TableArrays restates
seed and relax once more on whole numpy arrays, for batches the loop cannot follow (tests/large_case.py); tests/
test_table.py pins it to TableModel bit for bit.

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


class TableArrays:
    """TableModel on whole arrays: the same semantics (counting entries in ascending e; a node's id by first occurrence;
    g = min; the winner is the smallest e with cand == new g on an improved node; the state is that of the creating entry
    and is never rewritten), the same IEEE operations in the same order (cand = parent_g + cost, then + 0.0), the same
    return values.  The node arrays are attributes: hash, g, pred, pred_action [n_nodes], state [n_fields][n_nodes]."""

    def __init__(self, n_fields):
        self.n_fields = n_fields
        self.hash, self.g = np.zeros(0, np.uint64), np.zeros(0, np.float64)
        self.pred, self.pred_action = np.zeros(0, np.int32), np.zeros(0, np.int32)
        self.state = np.zeros((n_fields, 0), np.float64)
        self.counting = 0

    @property
    def n_nodes(self):
        return self.hash.size

    def arrays(self):
        return {"n_nodes": self.n_nodes, "hash": self.hash, "g": self.g, "pred": self.pred, "pred_action": self.pred_action,
                "state": self.state}

    def _walk(self, e, h, cand, pred, action, src_state, n_entries):
        """e: the counting entries, ascending; h, cand, pred, action: theirs; src_state[:, e]: their state columns."""
        n_old = self.n_nodes
        self.counting += e.size
        # ids by first occurrence: the known keys come first (they are distinct and keep their ids), then the entries
        _, first, inv = np.unique(np.concatenate([self.hash, h]), return_index=True, return_inverse=True)
        is_first = np.zeros(n_old + e.size, bool)
        is_first[first] = True
        created = np.nonzero(is_first[n_old:])[0]  # per new node, in id order: the position of its creating entry in e
        eid = (np.cumsum(is_first) - 1)[first[inv.ravel()[n_old:]]]
        n_new = created.size
        self.hash = np.concatenate([self.hash, h[created]])
        self.state = np.concatenate([self.state, src_state[:, e[created]]], axis=1)
        self.pred = np.concatenate([self.pred, np.full(n_new, -1, np.int32)])
        self.pred_action = np.concatenate([self.pred_action, np.full(n_new, -1, np.int32)])
        before = np.concatenate([self.g, np.full(n_new, np.inf)])
        self.g = before.copy()
        np.minimum.at(self.g, eid, cand)
        # improved nodes: the first entry (the smallest e) whose candidate is the new g
        at = np.nonzero((self.g < before)[eid] & (cand == self.g[eid]))[0]
        first_at = np.full(self.g.size, e.size, np.int64)
        np.minimum.at(first_at, eid[at], at)
        win = np.sort(first_at[first_at < e.size])  # the winning entries, in entry order
        wid = eid[win]
        self.pred[wid] = pred[win]
        self.pred_action[wid] = action[win]
        entry_id = np.full(n_entries, -1, np.int32)
        entry_id[e] = eid
        return {"count": wid.size, "id": wid.astype(np.int32), "g": self.g[wid], "state": self.state[:, wid]}, entry_id

    def seed(self, states, hashes, g=None):
        states = np.asarray(states, dtype=np.float64).reshape(self.n_fields, -1)
        n = states.shape[1]
        gs = np.zeros(n) if g is None else np.broadcast_to(np.asarray(g, dtype=np.float64), (n,))
        with np.errstate(invalid="ignore"):
            e = np.nonzero(np.isfinite(gs) & (gs >= 0.0))[0]
        none = np.full(e.size, -1, np.int32)
        return self._walk(e, np.asarray(hashes, dtype=np.uint64)[e], gs[e] + 0.0, none, none, states, n)

    def relax(self, lists, parent_id, parent_g, g_max=math.inf, n_nodes=None):
        S = int(lists["stride"])
        n = len(lists["count"]) if n_nodes is None else int(n_nodes)
        N = n * S
        count, pid = np.asarray(lists["count"][:n]), np.asarray(parent_id[:n])
        cost = np.asarray(lists["cost"][:N], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            cand = np.repeat(np.asarray(parent_g[:n], dtype=np.float64), S) + cost  # one IEEE add
            ok = (np.tile(np.arange(S), n) < np.repeat(count, S)) & np.repeat(pid >= 0, S) & np.isfinite(cost)
            ok &= np.isfinite(cand) & (cand >= 0.0) & (cand <= g_max)
        e = np.nonzero(ok)[0]
        return self._walk(e, np.asarray(lists["hash"][:N], dtype=np.uint64)[e], cand[e] + 0.0, np.repeat(pid, S)[e].astype(np.int32),
                          np.asarray(lists["action"][:N])[e].astype(np.int32), lists["state"], N)


# ---- the hand-built lists of tests/test_gpu_table.py (tests/test_table.py runs them through both models on the CPU)
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)  # the hash the table's key field cannot hold
F2 = 10                                # state rows in 2D


def hand_lists(rng, n, S, pool, poison_base, inf_rate=0.05, nan_rate=0.05):
    """Random lists over a pool of hashes: costs from a few dyadic values (equal candidates across parents are common),
    +inf and NaN costs sprinkled in, entries past count poisoned with NaN cost and hashes that exist nowhere else."""
    count = rng.integers(0, S + 1, size=n).astype(np.int32)
    count[:3] = [0, S, 1]
    N = n * S
    live = (np.arange(S)[None, :] < count[:, None]).ravel()
    hsh = pool[rng.integers(0, len(pool), size=N)].astype(np.uint64)
    cost = rng.choice([0.25, 0.5, 1.0, 1.5, 2.0], size=N)
    r = rng.random(N)
    cost[r < inf_rate] = np.inf
    cost[(r >= inf_rate) & (r < inf_rate + nan_rate)] = np.nan
    cost[~live] = np.nan
    hsh[~live] = (np.uint64(poison_base) + np.arange(N, dtype=np.uint64))[~live]
    state = rng.standard_normal((F2, N))
    state[:, ~live] = np.nan
    return {"stride": S, "count": count, "action": rng.integers(0, 25, size=N).astype(np.int32), "cost": cost, "hash": hsh,
            "state": state}


def hand_case(seed=11, n=300, S=40):
    rng = np.random.default_rng(seed)
    pool = np.concatenate([rng.integers(1, 2 ** 63, size=1500, dtype=np.uint64), np.full(12, EMPTY, np.uint64)])
    host = hand_lists(rng, n, S, pool, poison_base=0xDEAD00000000)
    parent_id = np.arange(1000, 1000 + n, dtype=np.int32)
    parent_id[7] = -1
    parent_g = rng.choice([0.0, 0.5, 1.0, 1.5, 2.5], size=n)
    return rng, pool, host, parent_id, parent_g


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
