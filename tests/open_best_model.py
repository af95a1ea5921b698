"""A plain sequential restatement of include/mplx_best.h over tests/open_model.py and tests/multi_model.py: the k best open
nodes per query are a sort by (bit pattern of f, id).  Test infrastructure: Python floats and dicts, nothing shared with
the engine."""
import math
import struct

import numpy as np

import multi_model as MM
import open_model as OM

IS_OPEN, IS_GOAL = OM.IS_OPEN, OM.IS_GOAL
SELECTED, FOUND, EMPTY, MAX_ROUNDS, MAX_EXPAND = OM.SELECTED, OM.FOUND, OM.EMPTY, OM.MAX_ROUNDS, OM.MAX_EXPAND


def key_bits(f):
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def k_best(f, cand, k):
    """The k first of `cand` (node ids) in the order (bit pattern of f, id); all of them when they are no more than k."""
    if k < 1:
        raise ValueError("k < 1")  # (MPLX_ERR_ARG on the device)
    if len(cand) <= k:
        return list(cand)
    return sorted(cand, key=lambda i: (key_bits(f[i]), i))[:k]


def _frontier(table, chosen):
    st = np.zeros((table.n_fields, len(chosen)))
    for r, i in enumerate(chosen):
        st[:, r] = table.state[i]
    return {"count": len(chosen), "id": np.array(chosen, dtype=np.int32),
            "g": np.array([table.g[i] for i in chosen], dtype=np.float64), "state": st}


class OpenBestModel(OM.OpenModel):
    def select_best(self, k, delta, capacity):
        """OpenModel.select with the k cut in front of the capacity cut."""
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
            chosen = sorted(k_best(self.f, [i for i in O if self.f[i] <= T], k))[:int(capacity)]
            for i in chosen:
                self.flags[i] &= ~IS_OPEN
        res = {"status": status, "goal_id": goal_id, "count": len(chosen), "n_open": len(O) - len(chosen), "f_min": f_min,
               "goal_f": goal_f, "goal_g": goal_g}
        return res, _frontier(self.table, chosen)


class MultiOpenBestModel(MM.MultiOpenModel):
    def select_best_many(self, k, delta, capacity):
        """MultiOpenModel.select_many with the k cut per query in front of the union and its capacity cut."""
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
                marked += k_best(self.f, [i for i in O if self.f[i] <= T], k)
            res.append({"status": status, "goal_id": goal_id, "count": 0, "n_open": len(O), "f_min": f_min, "goal_f": goal_f,
                        "goal_g": goal_g})
        chosen = sorted(marked)[:int(capacity)]
        for i in chosen:
            self.flags[i] &= ~IS_OPEN
            r = res[self.table.query[i]]
            r["count"] += 1
            r["n_open"] -= 1
        return res, _frontier(self.table, chosen)


def search_best(table, opn, provider, start, start_hash, eps, delta, k, capacity, g_max=math.inf, sight=0, on_round=None):
    """open_model.search with select_best.  Returns a dict: status, result (the last select's), rounds, expanded, nodes."""
    imp, _ = table.seed(start, [start_hash])
    opn.push(imp, imp["count"], eps, sight)
    rounds = expanded = 0
    while True:
        res, sel = opn.select_best(k, delta, capacity)
        if res["status"] != SELECTED:
            break
        lists = provider(sel["state"])
        imp, _ = table.relax(lists, sel["id"], sel["g"], g_max)
        opn.push(imp, sel["count"] * int(lists["stride"]), eps, sight)
        rounds += 1
        expanded += sel["count"]
        if on_round:
            on_round(rounds, sel, lists, imp)
    return {"status": res["status"], "result": res, "rounds": rounds, "expanded": expanded, "nodes": table.n_nodes}


def planted(states, keys, ids=None):
    """A frontier dict that plants keys[i] on node ids[i] of a table seeded with `states` when pushed with eps = 0
    (f = g), as the hand scenario of tests/test_gpu_open.py plants its keys."""
    keys = np.asarray(keys, dtype=np.float64)
    ids = np.arange(keys.size) if ids is None else np.asarray(ids)
    return {"count": int(ids.size), "id": ids.astype(np.int32), "g": keys, "state": np.asarray(states)[:, ids]}


def rest_states(n, width=128):
    """n distinct 2D ACC states at rest on a lattice of 0.1 m, `width` to a row."""
    s = np.zeros((10, n))
    i = np.arange(n)
    s[0], s[1] = (i % width) * 0.1, (i // width) * 0.1
    return s


# ---- the key patterns of tests/test_gpu_open_best.py: name -> (keys [n], delta)
PATTERN_N = 8229  # two tiles of 4 096 ids and 37: equal keys straddle tile, workgroup and wave boundaries
PATTERN_KS = (1, 63, 64, 65, 4096, 4097, 8228)


def key_patterns(n=PATTERN_N, seed=3):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    expo = np.concatenate([2.0 ** np.arange(-1022, 1024), [0.0, 5e-324, math.inf]])  # 2 049 distinct keys
    rnd = (rng.integers(0, 0x7ff0000000000000, size=n, dtype=np.uint64)).view(np.float64)  # finite, non-negative
    one_low, one_high = np.full(n, 2.0), np.full(n, 1.0)
    one_low[n // 3], one_high[n // 3] = 1.0, 2.0
    return {
        "equal": (np.full(n, 3.5), 0.0),
        "low_bits": ((1.0 + i * 2.0 ** -52)[rng.permutation(n)], 1.0),
        "exponents": (expo[i % expo.size][rng.permutation(n)], math.inf),
        "random": (rnd, math.inf),
        "one_below": (one_low, math.inf),
        "one_above": (one_high, math.inf),
    }
