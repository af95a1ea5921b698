"""The open set of a node table on the device (include/mplx_open.h) and the goal-directed search built on it.

    tab, opn = env.alloc_table(capacity), None
    opn = env.alloc_open(tab)
    env.set_goal(goal_row, tol_pos=0.5)
    count = tab.seed(start, frontier=imp)
    opn.push(imp, n_max=count, eps=1.0)
    while True:
        r = opn.select(delta, sel)                      # the round's only read-back
        if r["status"] != SELECTED: break
        env.expand_lists_resident(sel, lists, n_nodes=r["count"])
        tab.relax(lists, sel.id, sel.g, g_max, frontier=imp, n_nodes=r["count"], want_count=False)
        opn.push(imp, n_max=r["count"] * lists.stride, eps=1.0)

is EnvMap.search.  With a table of Q queries (include/mplx_multi.h), opn.set_goals(goal_rows) and opn.select_many the
same loop runs Q searches at once: EnvMap.search_many.
"""
import ctypes as C
import math

import numpy as np

from . import _abi
from .table import NodeTable, TableFrontier

IS_OPEN, IS_GOAL, SEEN = _abi.OPEN_IS_OPEN, _abi.OPEN_IS_GOAL, _abi.OPEN_SEEN
SELECTED, FOUND, EMPTY = _abi.OPEN_SELECTED, _abi.OPEN_FOUND, _abi.OPEN_EMPTY
# statuses of a SearchResult beyond those of a select: the search stopped at a limit with nodes still open
MAX_ROUNDS, MAX_EXPAND = 3, 4
STATUS_NAMES = {SELECTED: "SELECTED", FOUND: "FOUND", EMPTY: "EMPTY", MAX_ROUNDS: "MAX_ROUNDS", MAX_EXPAND: "MAX_EXPAND"}


class OpenSet:
    """mplx_open of a NodeTable.  Free it (or let it go) before the table."""

    def __init__(self, env, table):
        self._env = env
        self._table = table  # (kept alive: the open set reads the table's arrays)
        self._open = None
        self.capacity = table.capacity
        self.n_queries = getattr(table, "n_queries", 1)
        o = C.c_void_p()
        _abi.check(env._ctx, _abi.lib().mplx_open_create(table._tab, C.byref(o)))
        self._open = o

    def _check(self, rc):
        _abi.check(self._env._ctx, rc)

    def free(self):
        if self._open and self._env._ctx and self._table._tab:
            _abi.lib().mplx_open_destroy(self._open)
        self._open = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def clear(self):
        self._check(_abi.lib().mplx_open_clear(self._open))

    def push(self, frontier, n_max=None, eps=1.0, sight=False):
        """mplx_open_push_device: the first min(count on the device, n_max, capacity) rows of `frontier` become open
        with f = g + eps * h.  Asynchronous."""
        f = frontier.c_struct()
        n = frontier.capacity if n_max is None else int(n_max)
        self._check(_abi.lib().mplx_open_push_device(self._open, C.byref(f), n, float(eps), 1 if sight else 0))

    def select(self, delta, frontier, want_result=True, d_result=None):
        """mplx_open_select_device into `frontier`.  Returns the result as a dict (one synchronisation), or None with
        want_result=False -- the call is then asynchronous; d_result: a device buffer of 48 bytes, or None."""
        f = frontier.c_struct()
        r = _abi.OpenResult()
        self._check(_abi.lib().mplx_open_select_device(self._open, float(delta), C.byref(f),
                                                       d_result.ptr if d_result is not None else None,
                                                       C.byref(r) if want_result else None))
        if not want_result:
            return None
        return {"status": int(r.status), "goal_id": int(r.goal_id), "count": int(r.count), "n_open": int(r.n_open),
                "f_min": float(r.f_min), "goal_f": float(r.goal_f), "goal_g": float(r.goal_g)}

    def set_goals(self, goal_rows, w=None, v_max=None, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0, tol_yaw=-1.0, goal_control=0):
        """mplx_open_set_goals: goal_rows [Q][4D+2], one goal per query of the table; w, v_max and the tolerances as
        EnvMap.set_goal takes them, one value for all queries or [Q]."""
        env = self._env
        env._flush()
        rows = np.ascontiguousarray(goal_rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != env.n_fields:
            raise ValueError("goal_rows must be [Q][%d]" % env.n_fields)
        n = rows.shape[0]
        per = lambda v, default=None: np.broadcast_to(np.asarray(default if v is None else v, dtype=np.float64), (n,))
        ws, vs = per(w, env._p.w), per(v_max, env._p.v_max)
        tp, tv, ta, ty = per(tol_pos), per(tol_vel), per(tol_acc), per(tol_yaw)
        specs = (_abi.GoalSpec * max(n, 1))()
        for q in range(n):
            g = specs[q]
            g.goal, g.control, g.goal_control = rows[q].ctypes.data, int(env._p.control), int(goal_control)
            g.w, g.v_max = float(ws[q]), float(vs[q])
            g.tol_pos, g.tol_vel, g.tol_acc, g.tol_yaw = float(tp[q]), float(tv[q]), float(ta[q]), float(ty[q])
        self._check(_abi.lib().mplx_open_set_goals(self._open, specs, n))

    def select_many(self, delta, frontier, want_result=True, d_results=None):
        """mplx_open_select_multi_device into `frontier`.  Returns the Q results as a list of dicts (one
        synchronisation), or None with want_result=False; d_results: a device buffer of Q * 48 bytes, or None."""
        f = frontier.c_struct()
        res = (_abi.OpenResult * self.n_queries)()
        self._check(_abi.lib().mplx_open_select_multi_device(self._open, float(delta), C.byref(f),
                                                             d_results.ptr if d_results is not None else None,
                                                             res if want_result else None))
        if not want_result:
            return None
        return [{"status": int(r.status), "goal_id": int(r.goal_id), "count": int(r.count), "n_open": int(r.n_open),
                 "f_min": float(r.f_min), "goal_f": float(r.goal_f), "goal_g": float(r.goal_g)} for r in res]

    def view(self):
        v = _abi.OpenView()
        self._check(_abi.lib().mplx_open_view_of(self._open, C.byref(v)))
        return v

    def download(self):
        """f and flags of the table's nodes: {"n_nodes", "f", "flags"}; f is meaningful where flags has SEEN."""
        n = self._table.stats()[0]
        v = self.view()
        return {"n_nodes": n, "f": self._table._read(v.f, np.float64, n), "flags": self._table._read(v.flags, np.uint8, n)}


class SearchResult:
    """What EnvMap.search returns.  status: FOUND, EMPTY (no open node left: the goal region is not reachable within
    g_max), MAX_ROUNDS or MAX_EXPAND (stopped early; the nodes selected last are open again); cost: g of the goal node
    (inf unless FOUND); rounds = relax calls made; expanded = nodes expanded (a re-opened node counts again); table and
    open: the NodeTable and OpenSet, owned by the result -- free() it (or let it go) before the EnvMap is closed."""

    def __init__(self, status, last, table, open_set, rounds, expanded):
        self.status = status
        self.found = status == FOUND
        self.goal_id = last["goal_id"] if self.found else -1
        self.cost = last["goal_g"] if self.found else math.inf
        self.last_select = last
        self.table = table
        self.open = open_set
        self.rounds = rounds
        self.expanded = expanded

    def path(self):
        """(start_state, actions) of the chain of best predecessors from the seed to the goal node: the `starts` and
        `actions` (reshape(-1, 1)) of EnvMap.rollout / traj_*."""
        if not self.found:
            raise RuntimeError("search: no path (status %s)" % STATUS_NAMES[self.status])
        ids, act = self.table.path(self.goal_id)
        return self.table.state_of(ids[0]), act

    def free(self):
        self.open.free()
        self.table.free()

    def __repr__(self):
        return "SearchResult(%s, cost=%r, rounds=%d, expanded=%d)" % (STATUS_NAMES[self.status], self.cost, self.rounds, self.expanded)


def run_search(env, start, goal_row, eps, delta, g_max, max_rounds, max_expand, capacity, max_frontier, lists_stride, sight,
               tol_pos, tol_vel, tol_acc, tol_yaw, w, v_max):
    env._flush()
    if delta is None:
        delta = float(env._p.w) * float(env._p.dt)
    fcap = int(capacity if max_frontier is None else max_frontier)
    env.set_goal(goal_row, w=w, v_max=v_max, tol_pos=tol_pos, tol_vel=tol_vel, tol_acc=tol_acc, tol_yaw=tol_yaw)
    tab = NodeTable(env, capacity)
    opn = sel = imp = lists = None
    try:
        opn = OpenSet(env, tab)
        sel, imp = TableFrontier(env, fcap), TableFrontier(env, int(capacity))  # (no more nodes can improve than exist)
        lists = env.alloc_lists(fcap, want_state=True, stride=lists_stride)

        def check(where):
            status = tab.stats()[1]  # (the stream is idle: no copy, no wait)
            if status:
                raise RuntimeError("search: table status %d %s (1 nodes full, 2 probe full, 4 frontier full): raise capacity"
                                   % (status, where))
        count = tab.seed(start, frontier=imp)
        check("after seeding")
        opn.push(imp, n_max=count, eps=eps, sight=sight)
        rounds = expanded = 0
        while True:
            try:
                r = opn.select(delta, sel)
            except _abi.MplxError as e:
                if e.code != _abi.ERR_STATE:
                    raise
                check("in round %d" % rounds)
                raise
            status, n = r["status"], r["count"]
            if status != SELECTED:
                break
            limit = MAX_ROUNDS if (max_rounds is not None and rounds >= max_rounds) else \
                MAX_EXPAND if (max_expand is not None and expanded + n > max_expand) else None
            if limit is not None:
                opn.push(sel, n_max=n, eps=eps, sight=sight)  # the selection is open again: same g, same keys
                status = limit
                break
            env.expand_lists_resident(sel, lists, n_nodes=n)
            tab.relax(lists, sel.id, sel.g, g_max, frontier=imp, n_nodes=n, want_count=False)
            opn.push(imp, n_max=n * lists.stride, eps=eps, sight=sight)
            rounds += 1
            expanded += n
        return SearchResult(status, r, tab, opn, rounds, expanded)
    except Exception:
        if opn is not None:
            opn.free()
        tab.free()
        raise
    finally:
        for b in (sel, imp, lists):
            if b is not None:
                b.free()


class MultiSearchResult:
    """What EnvMap.search_many returns: per query q status[q] (FOUND, EMPTY, MAX_ROUNDS or MAX_EXPAND), found[q], cost[q]
    (inf unless FOUND), goal_id[q] (a global node id, -1 unless FOUND), rounds[q] (the rounds in which q selected) and
    expanded[q]; total_rounds = relax calls made.  last_select: the Q results of the last select.  table and open are
    owned by the result: free() it (or let it go) before the EnvMap is closed."""

    def __init__(self, status, last, table, open_set, rounds, expanded, total_rounds):
        self.n_queries = len(status)
        self.status = list(status)
        self.found = [st == FOUND for st in status]
        self.goal_id = [r["goal_id"] if ok else -1 for r, ok in zip(last, self.found)]
        self.cost = [r["goal_g"] if ok else math.inf for r, ok in zip(last, self.found)]
        self.last_select = last
        self.table = table
        self.open = open_set
        self.rounds = list(rounds)
        self.expanded = list(expanded)
        self.total_rounds = total_rounds

    def path(self, q):
        """(start_state, actions) of query q, as SearchResult.path."""
        if not self.found[q]:
            raise RuntimeError("search_many: no path for query %d (status %s)" % (q, STATUS_NAMES[self.status[q]]))
        ids, act = self.table.path(self.goal_id[q])
        return self.table.state_of(ids[0]), act

    def free(self):
        self.open.free()
        self.table.free()

    def __repr__(self):
        return "MultiSearchResult(%s, rounds=%d, expanded=%d)" % (
            [STATUS_NAMES[st] for st in self.status], self.total_rounds, sum(self.expanded))


def run_search_many(env, starts, goal_rows, eps, delta, g_max, max_rounds, max_expand, capacity, max_frontier, lists_stride,
                    sight, tol_pos, tol_vel, tol_acc, tol_yaw, w, v_max):
    env._flush()
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    goal_rows = np.ascontiguousarray(goal_rows, dtype=np.float64)
    if starts.ndim != 2 or goal_rows.ndim != 2 or starts.shape[0] != env.n_fields or goal_rows.shape != (starts.shape[1], env.n_fields):
        raise ValueError("search_many: starts must be [%d][Q] and goal_rows [Q][%d]" % (env.n_fields, env.n_fields))
    Q = starts.shape[1]
    if Q < 1:
        raise ValueError("search_many: no query")
    if delta is None:
        delta = float(env._p.w) * float(env._p.dt)
    fcap = int(capacity if max_frontier is None else max_frontier)
    tab = NodeTable(env, capacity, n_queries=Q)
    opn = sel = imp = lists = None
    try:
        opn = OpenSet(env, tab)
        opn.set_goals(goal_rows, w=w, v_max=v_max, tol_pos=tol_pos, tol_vel=tol_vel, tol_acc=tol_acc, tol_yaw=tol_yaw)
        sel, imp = TableFrontier(env, fcap), TableFrontier(env, int(capacity))  # (no more nodes can improve than exist)
        lists = env.alloc_lists(fcap, want_state=True, stride=lists_stride)

        def check(where):
            status = tab.stats()[1]  # (the stream is idle: no copy, no wait)
            if status:
                raise RuntimeError("search_many: table status %d %s (1 nodes full, 2 probe full, 4 frontier full): raise capacity"
                                   % (status, where))
        count = tab.seed(starts, frontier=imp, query=np.arange(Q, dtype=np.int32))
        check("after seeding")
        opn.push(imp, n_max=count, eps=eps, sight=sight)
        total = 0
        rounds, expanded = [0] * Q, [0] * Q
        limit = None
        while True:
            try:
                res = opn.select_many(delta, sel)
            except _abi.MplxError as e:
                if e.code != _abi.ERR_STATE:
                    raise
                check("in round %d" % total)
                raise
            n = sum(r["count"] for r in res)
            if not any(r["status"] == SELECTED for r in res):
                break
            limit = MAX_ROUNDS if (max_rounds is not None and total >= max_rounds) else \
                MAX_EXPAND if (max_expand is not None and sum(expanded) + n > max_expand) else None
            if limit is not None:
                opn.push(sel, n_max=n, eps=eps, sight=sight)  # the selection is open again: same g, same keys
                break
            env.expand_lists_resident(sel, lists, n_nodes=n)
            tab.relax(lists, sel.id, sel.g, g_max, frontier=imp, n_nodes=n, want_count=False)
            opn.push(imp, n_max=n * lists.stride, eps=eps, sight=sight)
            total += 1
            for q, r in enumerate(res):
                if r["status"] == SELECTED:
                    rounds[q] += 1
                    expanded[q] += r["count"]
        status = [limit if (r["status"] == SELECTED and limit is not None) else r["status"] for r in res]
        return MultiSearchResult(status, res, tab, opn, rounds, expanded, total)
    except Exception:
        if opn is not None:
            opn.free()
        tab.free()
        raise
    finally:
        for b in (sel, imp, lists):
            if b is not None:
                b.free()
