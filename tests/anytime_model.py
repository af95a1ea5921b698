"""A plain sequential restatement of include/mplx_anytime.h: the re-key of an open set and the lower bound of its open
nodes, and SearchResult.bound's arithmetic on top of it.  Test infrastructure: Python floats (IEEE doubles, no
contraction), dicts and lists, nothing shared with the engine.

The open set is any model of tests/open_model.py's family (OpenModel, MultiOpenModel, PriorOpenModel, HeurOpenModel, ...):
its f and flags dicts are what is re-keyed, and its heur_and_tol(node id, state column) IS "the h a push would compute
for a frontier row that holds the node" -- the rule of the header, word for word.  `h_of(node id, state column)` replaces it
where no such model exists (a goal field).  The table is anything with n_nodes, g [n_nodes], state (state[:, id] or
state[id] a column of 4D+2 rows, chosen by `column`) and, on a table of several queries, query [n_nodes].
"""
import math

IS_OPEN, IS_GOAL, SEEN = 1, 2, 4


def table_column(table, i):
    """The state rows of node i: tests/table_model.py keeps a list of columns, the stubs of the GPU tests an array."""
    s = table.state
    return s[i] if isinstance(s, list) else s[:, i]


def rekey(opn, eps, write=True, cut=None, n_queries=1, h_of=None, column=table_column):
    """mplx_open_rekey_device on the model `opn` (f, flags: dicts by node id) of opn.table.  cut: None or [n_queries].
    Returns the bounds: [n_queries] dicts lower, n_open, n_pruned, n_rekeyed."""
    eps = float(eps)
    if not eps >= 0.0 or math.isinf(eps):
        raise ValueError("eps")
    if cut is not None:
        cut = [float(c) for c in cut]
        if len(cut) != n_queries or any(not c >= 0.0 for c in cut):
            raise ValueError("cut")
    t = opn.table
    query = getattr(t, "query", None)
    out = [{"lower": math.inf, "n_open": 0, "n_pruned": 0, "n_rekeyed": 0} for _ in range(n_queries)]
    for i in range(int(t.n_nodes)):
        fl = opn.flags.get(i, 0)
        if not fl & SEEN:
            continue
        q = int(query[i]) if (query is not None and n_queries > 1) else 0
        s = column(t, i)
        h = float(h_of(i, s) if h_of is not None else opn.heur_and_tol(i, s)[0])
        g = float(t.g[i])
        L = g + h
        b = out[q]
        if fl & IS_OPEN:
            b["n_open"] += 1
            if L >= 0.0:
                b["lower"] = min(b["lower"], L + 0.0)
        if not write:
            continue
        f = g if eps == 0 else g + eps * h
        if f >= 0.0:
            opn.f[i] = f + 0.0
            b["n_rekeyed"] += 1
        if cut is not None and (fl & IS_OPEN) and cut[q] < math.inf and L >= cut[q]:
            opn.flags[i] = fl & ~IS_OPEN
            b["n_pruned"] += 1
    return out


def slack_of(w, v_max, tol_pos):
    return w * tol_pos / v_max if v_max > 0 else w * tol_pos


def bound(cost, lower_open, g_max, slack, certified, pruned_at=math.inf):
    """SearchResult.bound of one query from the re-key's lower; pruned_at: the smallest cut an improve pruned with."""
    lower = max(0.0, min(lower_open, g_max, pruned_at) - slack)
    ratio = math.nan
    if certified:
        ratio = cost / lower if lower > 0 else (1.0 if cost == 0 else math.inf)
    return {"cost": cost, "lower": lower, "slack": slack, "ratio": ratio, "certified": certified}


def improve(table, opn, provider, eps, delta, capacity, rounds=0, expanded=0, cut=None, g_max=math.inf, sight=0, max_rounds=None,
            max_expand=None):
    """SearchResult.improve on the models of one query: the re-key, then the loop of tests/open_model.py::search from its
    first select on (the same statements: select, and while SELECTED expand, relax, push).  rounds / expanded count on.
    Returns the dict of open_model.search plus "rekey"."""
    import open_model as OM

    info = rekey(opn, eps, True, cut, 1)
    r0, e0, truncated = rounds, expanded, 0
    while True:
        res, sel = opn.select(delta, capacity)
        status = res["status"]
        if status != OM.SELECTED:
            break
        if max_rounds is not None and rounds - r0 >= max_rounds:
            status = OM.MAX_ROUNDS
        elif max_expand is not None and expanded - e0 + sel["count"] > max_expand:
            status = OM.MAX_EXPAND
        if status != OM.SELECTED:
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
    return {"status": status, "result": res, "rounds": rounds, "expanded": expanded, "truncated": truncated, "rekey": info}


def wall_cells(dims, gap=4):
    """The small map of the anytime tests: a wall across x at the middle, open over `gap` cells at the low end of y (and
    all of z).  Cells in the map's own order ([z][y][x])."""
    import numpy as np
    shape = tuple(reversed(dims))
    c = np.zeros(shape, np.int8)
    c[..., dims[0] // 2] = 100
    if len(dims) == 2:
        c[:gap, dims[0] // 2] = 0
    else:
        c[:, :gap, dims[0] // 2] = 0
    return c.ravel()


def wall_query(dims):
    """(start position, goal position) on the 0.25 m lattice, on either side of the wall and away from its gap."""
    y = (dims[1] - 6) * 0.25
    rest = [2.0] * (len(dims) - 2)
    return [1.0, y] + rest, [(dims[0] - 4) * 0.25, y] + rest
