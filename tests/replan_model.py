"""A plain sequential restatement of include/mplx_replan.h over tests/table_model.py, tests/open_model.py and
tests/multi_model.py: the rebase of a node table (root, bad edge, kept, apply, frontier, result), the closed push, and
the loop of SearchResult.replan / MultiSearchResult.replan built on them.  Test infrastructure: dicts, lists and Python
floats, nothing shared with the engine.  The closure is found by walking chains (bounded by the number of nodes), not
by pointer doubling: the two must agree on every table.

An edge function maps (parent id, action) to (slot status, successor hash, cost) of that ONE pair on the map as it is
now; OracleEdges takes it from the CPU oracle (expand the parent, look at the slot of the action).
"""
import math

import numpy as np

import open_model as OM
from multi_model import MultiTableModel
from table_model import TableModel

SLOT_FINITE = 1
FRONTIER_FULL = 4


class OracleEdges:
    """edge(p, a) from the oracle's dense slots of the parents' states.  prepare(parents) expands many at once."""

    def __init__(self, O, oenv, table):
        self.O, self.oenv, self.table = O, oenv, table
        self.nU = int(oenv.U.shape[0])
        self.slots = {}

    def prepare(self, parents):
        todo = sorted(set(int(p) for p in parents) - set(self.slots))
        if not todo:
            return
        st = np.ascontiguousarray(np.array([self.table.state[p] for p in todo], dtype=np.float64).T)
        d = self.O.expand(self.oenv, st, want_state=False)
        for k, p in enumerate(todo):
            lo, hi = k * self.nU, (k + 1) * self.nU
            self.slots[p] = (d["status"][lo:hi].copy(), d["hash"][lo:hi].copy(), d["cost"][lo:hi].copy())

    def __call__(self, p, a):
        self.prepare([p])
        st, hs, co = self.slots[int(p)]
        return int(st[a]), int(hs[a]), float(co[a])


def table_from_arrays(d, n_queries=1):
    """A TableModel (MultiTableModel for n_queries > 1) holding the arrays of a download() / arrays()."""
    n, F = int(d["n_nodes"]), int(np.asarray(d["state"]).shape[0])
    t = MultiTableModel(F, n_queries) if n_queries > 1 else TableModel(F)
    t.hash = [int(h) for h in d["hash"][:n]]
    t.g = [float(x) for x in d["g"][:n]]
    t.pred = [int(x) for x in d["pred"][:n]]
    t.pred_action = [int(x) for x in d["pred_action"][:n]]
    t.state = [np.array(d["state"][:, i], dtype=np.float64) for i in range(n)]
    if n_queries > 1:
        t.query = [int(q) for q in d["query"][:n]]
        t.ids = {(q, h): i for i, (q, h) in enumerate(zip(t.query, t.hash))}
    else:
        t.ids = {h: i for i, h in enumerate(t.hash)}
    return t


def roots_of(table, root=-1, roots=None):
    """root(id) for every node."""
    query = getattr(table, "query", None)
    out = []
    for i in range(table.n_nodes):
        r = int(root) if roots is None else int(roots[query[i] if query else 0])
        finite = math.isfinite(table.g[i])
        out.append(finite and (i == r if r >= 0 else table.pred[i] == -1))
    return out


def bad_edges(table, is_root, edge, nU):
    """{id: bad(id)} for the non-root nodes with a predecessor that is a node."""
    todo = [i for i in range(table.n_nodes) if not is_root[i] and 0 <= table.pred[i] < table.n_nodes]
    if hasattr(edge, "prepare"):
        edge.prepare([table.pred[i] for i in todo if 0 <= table.pred_action[i] < nU])
    bad = {}
    for i in todo:
        p, a = table.pred[i], table.pred_action[i]
        if not 0 <= a < nU:
            bad[i] = True
            continue
        status, h, cost = edge(p, a)
        if status != SLOT_FINITE or h != int(table.hash[i]):
            bad[i] = True
            continue
        cand = float(np.float64(table.g[p]) + np.float64(cost))  # one IEEE add
        bad[i] = cand > table.g[i]
    return bad


def rebase(table, edge=None, nU=0, root=-1, roots=None, check_edges=True, capacity=None):
    """The rule of include/mplx_replan.h, applied to `table` in place.  Returns (frontier, result, status): status has
    FRONTIER_FULL when more nodes are kept than `capacity` rows (the frontier then holds the first `capacity`)."""
    n = table.n_nodes
    is_root = roots_of(table, root, roots)
    bad = bad_edges(table, is_root, edge, nU) if check_edges else {}
    bad.update({i: True for i in range(n) if not is_root[i] and table.pred[i] >= n})  # no node: bad whatever check_edges is
    kept = {}
    for i in range(n):
        chain, cur, dec = [], i, False
        for _ in range(n + 1):  # (a walk that has not ended after n steps is in a cycle: dropped)
            if cur in kept:
                dec = kept[cur]
                break
            if is_root[cur]:
                dec = True
                chain.append(cur)
                break
            if table.pred[cur] < 0 or bad.get(cur, False):
                dec = False
                chain.append(cur)
                break
            chain.append(cur)
            cur = table.pred[cur]
        for c in chain:
            kept[c] = dec
    for i in range(n):
        if not kept[i]:
            table.g[i], table.pred[i], table.pred_action[i] = math.inf, -1, -1
        elif is_root[i]:
            table.pred[i], table.pred_action[i] = -1, -1
    ids = [i for i in range(n) if kept[i]]
    result = {"n_kept": len(ids), "n_bad_edges": sum(1 for v in bad.values() if v), "n_roots": sum(is_root)}
    status = 0
    if capacity is not None and len(ids) > capacity:
        status, ids = FRONTIER_FULL, ids[:int(capacity)]
    st = np.zeros((table.n_fields, len(ids)))
    for r, i in enumerate(ids):
        st[:, r] = table.state[i]
    fr = {"count": len(ids), "id": np.array(ids, dtype=np.int32), "g": np.array([table.g[i] for i in ids], dtype=np.float64),
          "state": st}
    return fr, result, status


def push_closed(opn, fr, n_max, eps, sight=0, capacity=None):
    """mplx_open_push_closed_device: the push of the model, with IS_OPEN taken off what it wrote."""
    f0, fl0 = opn.f, opn.flags
    opn.f, opn.flags = {}, {}
    try:
        opn.push(fr, n_max, eps, sight, capacity)
    finally:
        f1, fl1 = opn.f, opn.flags
        opn.f, opn.flags = f0, fl0
    f0.update(f1)
    for i, v in fl1.items():
        fl0[i] = v & ~OM.IS_OPEN


def rows_of(fr, first, n):
    return {"count": n, "id": fr["id"][first:first + n], "g": fr["g"][first:first + n], "state": fr["state"][:, first:first + n]}


def replan(table, opn, provider, edge, nU, eps, delta, capacity, root=-1, roots=None, check_edges=True, g_max=math.inf, sight=0,
           max_rounds=None, max_expand=None):
    """The loop of SearchResult.replan (roots is None) / MultiSearchResult.replan on the model: rebase, clear, closed
    push, the forced round in chunks of `capacity` rows, then the rounds of the search.  `opn` carries the goal(s) to
    plan towards.  Returns a dict: status (one, or [Q]), result(s) of the last select, rounds / expanded (the forced
    chunks included; per query for roots), total_rounds, info (the rebase's result), kept (its frontier)."""
    multi = roots is not None
    Q = table.n_queries if multi else 1
    kept, info, status = rebase(table, edge, nU, root, roots, check_edges)
    assert status == 0
    opn.f, opn.flags = {}, {}
    push_closed(opn, kept, kept["count"], eps, sight)
    total, rounds, expanded = 0, [0] * Q, [0] * Q
    for first in range(0, kept["count"], capacity):
        n = min(capacity, kept["count"] - first)
        rows = rows_of(kept, first, n)
        lists = provider(rows["state"])
        imp, _ = table.relax(lists, rows["id"], rows["g"], g_max)
        opn.push(imp, n * int(lists["stride"]), eps, sight)
        total += 1
        per = np.bincount([table.query[int(i)] for i in rows["id"]], minlength=Q) if multi else [n]
        for q in range(Q):
            if per[q]:
                rounds[q] += 1
                expanded[q] += int(per[q])
    return _rounds(table, opn, provider, eps, delta, capacity, g_max, sight, max_rounds, max_expand, multi, total, rounds, expanded,
                   {"info": info, "kept": kept})


def _rounds(table, opn, provider, eps, delta, capacity, g_max, sight, max_rounds, max_expand, multi, total, rounds, expanded, out):
    """The rounds of a search from its first select on, counted on from total / rounds / expanded."""
    limit = None
    while True:
        if multi:
            res, sel = opn.select_many(delta, capacity)
        else:
            r, sel = opn.select(delta, capacity)
            res = [r]
        if not any(r["status"] == OM.SELECTED for r in res):
            break
        if max_rounds is not None and total >= max_rounds:
            limit = OM.MAX_ROUNDS
        elif max_expand is not None and sum(expanded) + sel["count"] > max_expand:
            limit = OM.MAX_EXPAND
        if limit is not None:
            opn.push(sel, sel["count"], eps, sight)
            break
        lists = provider(sel["state"])
        imp, _ = table.relax(lists, sel["id"], sel["g"], g_max)
        opn.push(imp, sel["count"] * int(lists["stride"]), eps, sight)
        total += 1
        for q, r in enumerate(res):
            if r["status"] == OM.SELECTED:
                rounds[q] += 1
                expanded[q] += r["count"]
    st = [limit if (r["status"] == OM.SELECTED and limit is not None) else r["status"] for r in res]
    if multi:
        out.update({"status": st, "results": res, "rounds": rounds, "expanded": expanded, "total_rounds": total})
    else:
        out.update({"status": st[0], "result": res[0], "rounds": total, "expanded": expanded[0], "total_rounds": total})
    return out


def fresh(table, opn, provider, starts, start_hashes, start_g, eps, delta, capacity, g_max=math.inf, sight=0, multi=False):
    """EnvMap.search(..., start_g=g) / search_many on the model: what a replan is compared against.  starts [4D+2][Q]."""
    starts = np.asarray(starts, dtype=np.float64).reshape(table.n_fields, -1)
    Q = starts.shape[1]
    g = np.broadcast_to(np.asarray(start_g, dtype=np.float64), (Q,))
    imp, _ = table.seed(starts, start_hashes, g, query=np.arange(Q)) if multi else table.seed(starts, start_hashes, g)
    opn.push(imp, imp["count"], eps, sight)
    return _rounds(table, opn, provider, eps, delta, capacity, g_max, sight, None, None, multi, 0, [0] * Q, [0] * Q, {})


def path_ids(table, goal_id):
    """The chain of best predecessors from the seed to goal_id, root first."""
    ids, i = [int(goal_id)], int(goal_id)
    while table.pred[i] >= 0:
        i = table.pred[i]
        ids.append(i)
    return ids[::-1]


def wall_cells(map_dim, origin, res, a, b, length=7):
    """Cell indices (x + dim0 * y) of a wall `length` cells long and one thick, centred on the midpoint of the edge from
    position a to position b, perpendicular to the axis along which the edge moves more; cells outside the map left out."""
    a, b = np.asarray(a, dtype=np.float64)[:2], np.asarray(b, dtype=np.float64)[:2]
    mid = (a + b) / 2
    c = np.floor((mid - np.asarray(origin, dtype=np.float64)[:2]) / res).astype(int)
    along = 0 if abs(b[0] - a[0]) >= abs(b[1] - a[1]) else 1
    out = []
    for k in range(-(length // 2), length // 2 + 1):
        cell = c.copy()
        cell[1 - along] += k
        if 0 <= cell[0] < map_dim[0] and 0 <= cell[1] < map_dim[1]:
            out.append(int(cell[0] + map_dim[0] * cell[1]))
    return out
