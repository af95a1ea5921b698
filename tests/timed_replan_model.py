"""A plain sequential restatement of include/mplx_replan_timed.h on top of tests/replan_model.py (roots, the closed push),
tests/reserve_model.py (instants, horizon, pair test, time keys) and tests/wait_model.py (the pair, the wait's
eligibility and cost, the park veto, the open model): the edge rule with key fold and wait rule, the per-node
reservation test with `hit`, the rebase built on both, and the loop of SearchResult.replan_timed /
MultiSearchResult.replan_timed.  Test infrastructure: dicts, lists and numpy float64, nothing shared with the engine.

Tables are MultiTableModel throughout (a table of one query has the query column all 0), so one loop serves both
result classes.  An edge function maps (parent id, action) to (slot status, successor lattice hash, cost) of that ONE
pair on the map as it is now (replan_model.OracleEdges, or a hand-made one)."""
import math

import numpy as np

import multi_model as MM
import replan_model as RP
import reserve_model as RM
import wait_model as WM

F = np.float64
NO_HIT, HORIZON = RM.NO_HIT, RM.HORIZON
FRONTIER_FULL = RP.FRONTIER_FULL


class Config:
    """What the context holds: dim, control flag, U [nU][udim], dt, w, limits = (v_max, a_max, j_max, yaw_max)."""

    def __init__(self, dim, control, U, dt, w, limits=(0.0, 0.0, 0.0, 0.0)):
        self.dim, self.control, self.U, self.dt, self.w, self.limits = dim, control, np.asarray(U, dtype=F), float(dt), float(w), limits
        self.K = WM.order_of(control)
        self.nU = len(self.U)
        self.a0 = WM.zero_action(self.U)


def multi_table(d, n_queries=1):
    """A MultiTableModel holding the arrays of a download() / arrays() (query: zeros where there is none)."""
    n, nf = int(d["n_nodes"]), int(np.asarray(d["state"]).shape[0])
    t = MM.MultiTableModel(nf, n_queries)
    t.hash = [int(h) for h in d["hash"][:n]]
    t.g = [float(x) for x in d["g"][:n]]
    t.pred = [int(x) for x in d["pred"][:n]]
    t.pred_action = [int(x) for x in d["pred_action"][:n]]
    t.state = [np.array(np.asarray(d["state"])[:, i], dtype=F) for i in range(n)]
    t.query = [int(q) for q in d["query"][:n]] if "query" in d else [0] * n
    t.ids = {(q, h): i for i, (q, h) in enumerate(zip(t.query, t.hash))}
    return t


# ---------------------------------------------------------------------------------------------------- the edge rule
def edge_is_bad(table, i, edge, cfg, time_keys, allow_wait):
    """bad(i) by the ordinary-edge and wait-edge rules, for a non-root i with pred in [0, n)."""
    p, a = table.pred[i], table.pred_action[i]
    if not 0 <= a < cfg.nU:
        return True
    tp = F(table.state[p][-1])
    tc = tp + F(cfg.dt)  # one IEEE add
    pe = WM.pair_eval(cfg.dim, cfg.control, table.state[p], cfg.U[a], cfg.dt, *cfg.limits) if a == cfg.a0 else None
    if pe is not None and pe["h_next"] == pe["h_curr"]:  # a wait edge
        holds = bool(allow_wait) and pe["valid"] and pe["same_pos"]
        h, cost = pe["h_next"], 0.0 + (pe["J"] + cfg.w * cfg.dt)
    else:
        status, h, cost = edge(p, a)
        holds = status == RP.SLOT_FINITE
    if not holds:
        return True
    key = RM.time_key(h, float(tc)) if time_keys else int(h)
    if key != int(table.hash[i]):
        return True
    cand = float(F(table.g[p]) + F(cost))  # one IEEE add
    return cand > table.g[i]


def bad_edges(table, is_root, edge, cfg, time_keys, allow_wait):
    n = table.n_nodes
    todo = [i for i in range(n) if not is_root[i] and table.pred[i] >= 0]
    if hasattr(edge, "prepare"):
        edge.prepare([table.pred[i] for i in todo if table.pred[i] < n and 0 <= table.pred_action[i] < cfg.nU])
    return {i: (table.pred[i] >= n or edge_is_bad(table, i, edge, cfg, time_keys, allow_wait)) for i in todo}


# ---------------------------------------------------------------------------------------------------- reservations
def edge_position(table, cfg, p, a, s):
    """traj::eval_segment (positions only) of the segment of (state[p], U[a]) at local time s."""
    st, D, z = table.state[p], cfg.dim, np.zeros(cfg.dim)
    return RM.primitive_pos(st[:D], st[D:2 * D] if cfg.K >= 2 else z, st[2 * D:3 * D] if cfg.K >= 3 else z,
                            st[3 * D:4 * D] if cfg.K >= 4 else z, cfg.U[a][:D], cfg.K, s)


def reserve_hits(table, is_root, cfg, res, queries, n_steps, edge_pos=None):
    """hit [n] int64 of the per-node reservation test: res the dict of Reservations.positions() with "step", queries
    (t0 [Q], radius [Q], ignore [Q]).  edge_pos(p, a, i, s) -> [D] replaces the closed form (the device's own samples)."""
    n = table.n_nodes
    q_t0, q_r, q_ign = (np.asarray(x) for x in queries)
    Q = len(q_t0)
    step = F(res["step"])
    pos, act = np.asarray(res["pos"], dtype=F), np.asarray(res["active"]) != 0
    inc, r_b, g_b = np.asarray(res["included"]) != 0, np.asarray(res["radius"], dtype=F), np.asarray(res["group"])
    hit = np.full(n, NO_HIT, np.int64)
    for i_d in range(n):
        p, a = table.pred[i_d], table.pred_action[i_d]
        q = table.query[i_d]
        if is_root[i_d] or not 0 <= p < n or not 0 <= a < cfg.nU or not 0 <= q < Q:
            continue
        tp = F(table.state[p][-1])
        tc = tp + F(cfg.dt)
        if RM.leaves_horizon(step, n_steps, q_t0[q], tc):
            hit[i_d] = HORIZON
            continue
        on_q = inc & (g_b != q_ign[q])
        rr = F(q_r[q]) + r_b
        rr2 = rr * rr
        for i in RM.instants(step, n_steps, q_t0[q], tp, tc):
            tl = F(i) * step - F(q_t0[q])
            pt = np.asarray(edge_position(table, cfg, p, a, tl - tp) if edge_pos is None else edge_pos(p, a, int(i), tl - tp), dtype=F)
            with np.errstate(invalid="ignore", over="ignore"):
                d2 = None
                for d in range(cfg.dim):
                    dx = pt[d] - pos[i, d]
                    d2 = dx * dx if d2 is None else d2 + dx * dx
                conf = on_q & act[i] & (d2 < rr2)  # (a NaN compares false)
            if conf.any():
                hit[i_d] = (int(i) << 32) | int(np.argmax(conf))
                break
    return hit


# ---------------------------------------------------------------------------------------------------- the rebase
def rebase_timed(table, edge, cfg, roots, check_edges=True, allow_wait=False, time_keys=True, res=None, queries=None, n_steps=None,
                 capacity=None, edge_pos=None):
    """mplx_table_rebase_timed_device on `table` in place.  Returns (frontier, result, hit or None, n_blocked, status)."""
    n = table.n_nodes
    is_root = RP.roots_of(table, -1, roots)
    bad = bad_edges(table, is_root, edge, cfg, time_keys, allow_wait) if check_edges else {}
    hit, n_blocked = None, 0
    if res is not None:
        hit = reserve_hits(table, is_root, cfg, res, queries, n_steps, edge_pos)
        n_blocked = int((hit != NO_HIT).sum())
        for i in np.nonzero(hit != NO_HIT)[0]:
            bad[int(i)] = True
    kept = {}
    for i in range(n):
        chain, cur, dec = [], i, False
        for _ in range(n + 1):  # (a walk that has not ended after n steps is in a cycle: dropped)
            if cur in kept:
                dec = kept[cur]
                break
            chain.append(cur)
            if is_root[cur]:
                dec = True
                break
            if not 0 <= table.pred[cur] < n or bad.get(cur, False):
                dec = False
                break
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
    fr = {"count": len(ids), "id": np.array(ids, dtype=np.int32), "g": np.array([table.g[i] for i in ids], dtype=F), "state": st}
    return fr, result, hit, n_blocked, status


# ---------------------------------------------------------------------------------------------------- the loops
def timed_lists(provider, cfg, table, ids, states, wait, time_keys, res, queries, n_steps):
    """The lists of one expansion as the relax sees them: the provider's, the waits appended, the entries the check
    blocks at +inf, the hashes folded with the entries' t rows."""
    states = np.asarray(states, dtype=F)
    n = states.shape[1]
    lists = provider(states)
    S = int(lists["stride"])
    if wait:
        WM.add_wait(lists, n, states, None, cfg.dim, cfg.control, cfg.U, cfg.dt, cfg.w, *cfg.limits)
    if res is not None:
        row_q = np.array([table.query[int(i)] for i in ids], np.int32)

        def edge_pos(k, j, i, s):
            st, D, z = states[:, k], cfg.dim, np.zeros(cfg.dim)
            u = cfg.U[int(lists["action"][k * S + j])][:D]
            return RM.primitive_pos(st[:D], st[D:2 * D] if cfg.K >= 2 else z, st[2 * D:3 * D] if cfg.K >= 3 else z,
                                    st[3 * D:4 * D] if cfg.K >= 4 else z, u, cfg.K, s)
        lists["cost"] = RM.check(lists["count"], lists["action"], lists["cost"], S, np.zeros(n, np.int32), states[-1], cfg.dt, cfg.nU,
                                 res["step"], n_steps, res, queries, edge_pos, row_q)[0]
    if time_keys:
        for k in range(n):
            for j in range(int(lists["count"][k])):
                e = k * S + j
                lists["hash"][e] = RM.time_key(int(lists["hash"][e]), float(lists["state"][-1, e]))
    return lists


def _rounds(table, opn, expand, eps, delta, capacity, g_max, max_rounds, total, rounds, expanded, out):
    """The rounds of a search from its first select on (replan_model._rounds with the ids handed to the expansion)."""
    limit = None
    while True:
        res, sel = opn.select_many(delta, capacity)
        if not any(r["status"] == MM.SELECTED for r in res):
            break
        if max_rounds is not None and total >= max_rounds:
            limit = MM.MAX_ROUNDS
            opn.push(sel, sel["count"], eps)
            break
        lists = expand(sel["id"], sel["state"])
        imp, _ = table.relax(lists, sel["id"], sel["g"], g_max)
        opn.push(imp, sel["count"] * int(lists["stride"]), eps)
        total += 1
        for q, r in enumerate(res):
            if r["status"] == MM.SELECTED:
                rounds[q] += 1
                expanded[q] += r["count"]
    st = [limit if (r["status"] == MM.SELECTED and limit is not None) else r["status"] for r in res]
    out.update({"status": st, "results": res, "rounds": rounds, "expanded": expanded, "total_rounds": total})
    return out


def open_model(table, cfg, goal_rows, res, queries, park_goal, v_max_heur=1.0, tol_pos=0.5):
    """The open set of a search among reservations: the park veto after every push; with time keys no key equals the
    goal's own lattice hash, as on the device."""
    Q = table.n_queries
    opn = WM.ParkOpenModel(table, cfg.dim, goal_rows, [-1] * Q, w=cfg.w, v_max=v_max_heur, tol_pos=tol_pos, res=res, queries=queries,
                           park_goal=park_goal)
    return opn


def fresh(provider, cfg, starts, start_hashes, start_g, goal_rows, res, queries, n_steps, wait, park_goal, eps=1.0, delta=0.0,
          capacity=1 << 16, g_max=math.inf, max_rounds=None, time_keys=True):
    """EnvMap.search_many(avoid=, time_keys=True, wait=, park_goal=, start_g=) on the models: what a timed replan is
    compared against.  starts [4D+2][Q], start_hashes [Q] lattice hashes.  Returns (out, table, open model)."""
    starts = np.asarray(starts, dtype=F)
    Q = starts.shape[1]
    table = MM.MultiTableModel(4 * cfg.dim + 2, Q)
    opn = open_model(table, cfg, goal_rows, res, queries, park_goal)
    keys = [RM.time_key(int(h), float(starts[-1, q])) if time_keys else int(h) for q, h in enumerate(start_hashes)]
    g = np.broadcast_to(np.asarray(start_g, dtype=F), (Q,))
    imp, _ = table.seed(starts, keys, g, query=np.arange(Q))
    opn.push(imp, imp["count"], eps)
    expand = lambda ids, st: timed_lists(provider, cfg, table, ids, st, wait, time_keys, res, queries, n_steps)
    out = _rounds(table, opn, expand, eps, delta, capacity, g_max, max_rounds, 0, [0] * Q, [0] * Q, {})
    return out, table, opn


def replan_timed(table, opn, provider, edge, cfg, roots, res, queries, n_steps, wait, park_goal, eps=1.0, delta=0.0, capacity=1 << 16,
                 check_edges=True, g_max=math.inf, max_rounds=None, time_keys=True, executed=None):
    """The loop of replan_timed on the models.  opn: a ParkOpenModel of `table` (its reservation table and queries are
    replaced by res / queries).  executed: per query (start state, actions) so far, or None.  Returns a dict: status
    [Q], results, rounds, expanded, total_rounds, info, n_blocked, hit, kept, executed [Q]."""
    Q = table.n_queries
    done = list(executed) if executed is not None else [None] * Q
    for q, r in enumerate(roots):
        if 0 <= r < table.n_nodes:
            ids, acts = WM.path_of(table, r)
            if done[q] is None:
                done[q] = (np.array(table.state[ids[0]]), [])
            done[q] = (done[q][0], list(done[q][1]) + acts)
    kept, info, hit, n_blocked, status = rebase_timed(table, edge, cfg, roots, check_edges, wait, time_keys, res, queries, n_steps)
    assert status == 0
    opn.res, opn.queries, opn.park_goal = res, queries, bool(park_goal) and res is not None
    opn.f, opn.flags = {}, {}
    RP.push_closed(opn, kept, kept["count"], eps)
    expand = lambda ids, st: timed_lists(provider, cfg, table, ids, st, wait, time_keys, res, queries, n_steps)
    total, rounds, expanded = 0, [0] * Q, [0] * Q
    for first in range(0, kept["count"], capacity):
        n = min(capacity, kept["count"] - first)
        rows = RP.rows_of(kept, first, n)
        lists = expand(rows["id"], rows["state"])
        imp, _ = table.relax(lists, rows["id"], rows["g"], g_max)
        opn.push(imp, n * int(lists["stride"]), eps)
        total += 1
        per = np.bincount([table.query[int(i)] for i in rows["id"]], minlength=Q)
        for q in range(Q):
            if per[q]:
                rounds[q] += 1
                expanded[q] += int(per[q])
    out = {"info": info, "n_blocked": n_blocked, "hit": hit, "kept": kept, "executed": done}
    return _rounds(table, opn, expand, eps, delta, capacity, g_max, max_rounds, total, rounds, expanded, out)


def full_path(table, out, q):
    """(start state, actions) from the original start: the executed part, then the chain from the root to the goal."""
    ids, acts = WM.path_of(table, out["results"][q]["goal_id"])
    done = out["executed"][q]
    if done is None:
        return np.array(table.state[ids[0]]), acts
    return done[0], list(done[1]) + acts
