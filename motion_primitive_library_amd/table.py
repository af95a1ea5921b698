"""The persistent node table on the device (include/mplx_table.h): the nodes of a search with their g values and best
back-pointers, the relaxation of whole batches of successor lists against them, and the next frontier.

    tab = env.alloc_table(capacity)
    cur, nxt = env.alloc_table_frontier(n), env.alloc_table_frontier(n)
    count = tab.seed(starts, frontier=cur)
    while count:
        env.expand_lists_resident(cur, lists, n_nodes=count)
        count = tab.relax(lists, cur.id, cur.g, frontier=nxt, n_nodes=count)
        cur, nxt = nxt, cur

is EnvMap.cost_to_come: a label-correcting sweep that stays on the device but for one 8-byte count per round.
"""
import ctypes as C

import numpy as np

from . import _abi
from .env import DeviceArray, _device_ptr

NODES_FULL, PROBE_FULL, FRONTIER_FULL = _abi.TABLE_NODES_FULL, _abi.TABLE_PROBE_FULL, _abi.TABLE_FRONTIER_FULL


class TableFrontier:
    """Caller-owned frontier rows (mplx_table_frontier): id, g, state [4D+2][state_stride] and the count.  `ptr` /
    `n_nodes` make it the `frontier` argument of EnvMap.expand_lists_resident (its state rows, state_stride entries
    apart).  spare: entries allocated behind `capacity` in every row that no call may touch (tests look at them)."""

    def __init__(self, env, capacity, spare=0):
        self._env = env
        self.capacity = int(capacity)
        self.state_stride = max(self.capacity + int(spare), 1)
        self.n_fields = env.n_fields
        n = self.state_stride
        self.id = DeviceArray(env, n * 4)
        self.g = DeviceArray(env, n * 8)
        self.state = DeviceArray(env, n * 8 * self.n_fields)
        self.count = DeviceArray(env, 8)

    @property
    def ptr(self):
        return self.state.ptr

    @property
    def n_nodes(self):
        return self.state_stride

    def c_struct(self):
        f = _abi.TableFrontier()
        f.id, f.g, f.state, f.count = self.id.ptr, self.g.ptr, self.state.ptr, self.count.ptr
        f.state_stride, f.capacity = self.state_stride, self.capacity
        return f

    def download(self, count=None):
        """The first `count` rows (default: the count on the device) as numpy arrays."""
        n = int(self.count.download(np.int64, (1,))[0]) if count is None else int(count)
        st = self.state.download(np.float64, (self.n_fields, self.state_stride))
        return {"count": n, "id": self.id.download(np.int32, (n,)), "g": self.g.download(np.float64, (n,)),
                "state": np.ascontiguousarray(st[:, :n])}

    def free(self):
        for b in (self.id, self.g, self.state, self.count):
            b.free()

    def rows(self, first, n):
        """Rows [first, first + n) as the `frontier` of EnvMap.expand_lists_resident and, through .id / .g, as the
        parent_id / parent_g of NodeTable.relax: a view, valid while this frontier is."""
        first, n = int(first), int(n)
        if first < 0 or n < 0 or first + n > self.state_stride:
            raise ValueError("rows [%d, %d) of a frontier of %d" % (first, first + n, self.state_stride))
        return _FrontierRows(self, first)


class _Ptr:
    def __init__(self, ptr):
        self.ptr = ptr


class _FrontierRows:
    def __init__(self, frontier, first):
        self._frontier = frontier  # (kept alive)
        self.id, self.g = _Ptr(frontier.id.ptr + 4 * first), _Ptr(frontier.g.ptr + 8 * first)
        self.ptr = frontier.state.ptr + 8 * first
        self.n_nodes = frontier.state_stride


class NodeTable:
    """mplx_table of an EnvMap's context.  Free it (or let it go) before the EnvMap is closed.  n_queries > 1: a table
    of that many queries (include/mplx_multi.h): a node is a (query, hash) pair, slots_log2 sizes one query's region of
    the hash table, seed / find take the query of every state / hash."""

    _roots = None  # device copy of the roots of a rebase, allocated by the first one that needs it

    def __init__(self, env, capacity, slots_log2=0, n_queries=1):
        self._env = env
        self._tab = None
        self.capacity = int(capacity)
        self.n_queries = int(n_queries)
        self.n_fields = env.n_fields
        t = C.c_void_p()
        if self.n_queries == 1:
            rc = _abi.lib().mplx_table_create(env._ctx, self.capacity, int(slots_log2), C.byref(t))
        else:
            rc = _abi.lib().mplx_table_create_multi(env._ctx, self.capacity, self.n_queries, int(slots_log2), C.byref(t))
        _abi.check(env._ctx, rc)
        self._tab = t

    def _check(self, rc):
        _abi.check(self._env._ctx, rc)

    def free(self):
        tab, roots = self._tab, self._roots
        self._tab, self._roots = None, None  # (first: whatever happens below, nothing is destroyed twice)
        if tab and self._env._ctx:
            _abi.lib().mplx_table_destroy(tab)
            if roots is not None:
                roots.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def clear(self):
        self._check(_abi.lib().mplx_table_clear(self._tab))

    def set_time_keys(self, on=True):
        """mplx_table_set_time_keys: a node's key is combine(hash, round(t / 0.1)); an empty table only."""
        self._check(_abi.lib().mplx_table_set_time_keys(self._tab, 1 if on else 0))

    def stats(self):
        """(number of nodes, status bits); synchronises."""
        n, st = C.c_int64(), C.c_uint32()
        self._check(_abi.lib().mplx_table_stats(self._tab, C.byref(n), C.byref(st)))
        return int(n.value), int(st.value)

    def seed(self, states, g=None, frontier=None, query=None):
        """Creates / improves the nodes of `states` ([4D+2][n] or one state) with cost-to-come g (default 0) and no
        predecessor; writes the first frontier.  Returns the frontier count (and the frontier it allocated, if none
        was given: (count, frontier)).  query: the query of every state ([n] or one for all; mplx_table_seed_multi);
        None is the plain call, which a table of several queries refuses."""
        self._env._flush()
        states = np.ascontiguousarray(states, dtype=np.float64)
        if states.ndim == 1:
            states = np.ascontiguousarray(states.reshape(-1, 1))
        if states.ndim != 2 or states.shape[0] != self.n_fields:
            raise ValueError("states must be [%d][n]" % self.n_fields)
        n = states.shape[1]
        gp = None
        if g is not None:
            g = np.ascontiguousarray(np.broadcast_to(np.asarray(g, dtype=np.float64), (n,)))
            gp = g.ctypes.data
        own = frontier is None
        if own:
            frontier = TableFrontier(self._env, n)
        f = frontier.c_struct()
        cnt = C.c_int64(-1)
        if query is None:
            self._check(_abi.lib().mplx_table_seed(self._tab, states.ctypes.data, n, n, gp, C.byref(f), C.byref(cnt)))
        else:
            q = np.ascontiguousarray(np.broadcast_to(np.asarray(query, dtype=np.int32), (n,)))
            self._check(_abi.lib().mplx_table_seed_multi(self._tab, states.ctypes.data, n, n, gp, q.ctypes.data, C.byref(f),
                                                         C.byref(cnt)))
        return (int(cnt.value), frontier) if own else int(cnt.value)

    def relax(self, lists, parent_id, parent_g, g_max=float("inf"), frontier=None, n_nodes=None, entry_id=None, want_count=True):
        """mplx_table_relax_device on HBM-resident lists.  parent_id / parent_g: device buffers (a frontier's id / g).
        entry_id: a device buffer of lists.n_slots int32, or None.  Returns the count of `frontier` (one 8-byte
        read-back) or, with want_count=False, None -- the call is then asynchronous."""
        if frontier is None:
            raise ValueError("relax needs a frontier to write (EnvMap.alloc_table_frontier)")
        n = lists.n_nodes if n_nodes is None else int(n_nodes)
        s, f = lists.c_struct(), frontier.c_struct()
        cnt = C.c_int64(-1)
        self._check(_abi.lib().mplx_table_relax_device(
            self._tab, C.byref(s), n, _device_ptr(parent_id), _device_ptr(parent_g), float(g_max), C.byref(f),
            _device_ptr(entry_id) if entry_id is not None else None, C.byref(cnt) if want_count else None))
        return int(cnt.value) if want_count else None

    def rebase(self, root=-1, roots=None, check_edges=True, frontier=None, want_result=True):
        """mplx_table_rebase_device (include/mplx_replan.h): keeps the nodes that hang below `root` (a node id; -1: the
        seeds) by edges that still hold on the map the context has now, resets every other node to "never reached" and
        writes the kept nodes to `frontier` in id order.  roots: one root per query ([Q], -1 = that query's seeds;
        mplx_table_rebase_multi_device) -- a table of several queries needs it.  check_edges=False keeps every edge.
        Returns {"n_kept", "n_bad_edges", "n_roots"} (one synchronisation) or, with want_result=False, None -- the call
        is then asynchronous."""
        if frontier is None:
            raise ValueError("rebase needs a frontier to write (EnvMap.alloc_table_frontier)")
        self._env._flush()
        f = frontier.c_struct()
        r = _abi.RebaseResult()
        rp = C.byref(r) if want_result else None
        if roots is None:
            self._check(_abi.lib().mplx_table_rebase_device(self._tab, int(root), 1 if check_edges else 0, C.byref(f), None, rp))
        else:
            h = np.ascontiguousarray(np.broadcast_to(np.asarray(roots, dtype=np.int32), (self.n_queries,)))
            if self._roots is None:
                self._roots = DeviceArray(self._env, 4 * self.n_queries)
            self._roots.upload(h)
            self._check(_abi.lib().mplx_table_rebase_multi_device(self._tab, self._roots.ptr, 1 if check_edges else 0, C.byref(f),
                                                                  None, rp))
        if not want_result:
            return None
        return {"n_kept": int(r.n_kept), "n_bad_edges": int(r.n_bad_edges), "n_roots": int(r.n_roots)}

    def rebase_timed(self, roots, check_edges=True, allow_wait=False, avoid=None, frontier=None, want_hit=False, want_result=True):
        """mplx_table_rebase_timed_device (include/mplx_replan_timed.h): rebase(roots=) for a table with time keys, wait
        edges and reservations.  roots: one root per query ([Q] or one for all; -1 = that query's seeds).  An edge is bad
        as rebase() has it -- the identity test on the time key where the table has time keys, a wait edge held by the
        wait's eligibility and cost if allow_wait, bad otherwise -- or, with avoid (a Reservations, filled and with its
        queries set), if it comes too close to a reservation or leaves the table's horizon.  Returns {"n_kept",
        "n_bad_edges", "n_roots"}, with avoid also "n_blocked", with want_hit also "hit" (int64 [n_nodes]: the smallest
        (i << 32 | b) of the edge's conflicts, -2 for the horizon, -1) (one synchronisation); None with
        want_result=False -- the call is then asynchronous."""
        if frontier is None:
            raise ValueError("rebase_timed needs a frontier to write (EnvMap.alloc_table_frontier)")
        if want_hit and not want_result:
            raise ValueError("rebase_timed: want_hit needs want_result")
        self._env._flush()
        f = frontier.c_struct()
        r = _abi.RebaseResult()
        h = np.ascontiguousarray(np.broadcast_to(np.asarray(roots, dtype=np.int32), (self.n_queries,)))
        if self._roots is None:
            self._roots = DeviceArray(self._env, 4 * self.n_queries)
        self._roots.upload(h)
        hit = blocked = None
        try:
            if avoid is not None and want_result:
                blocked = DeviceArray(self._env, 8)
                blocked.upload(np.zeros(1, np.int64))
                if want_hit:
                    hit = DeviceArray(self._env, 8 * self.capacity)
            self._check(_abi.lib().mplx_table_rebase_timed_device(
                self._tab, self._roots.ptr, 1 if check_edges else 0, 1 if allow_wait else 0, None if avoid is None else avoid._res,
                C.byref(f), None if hit is None else hit.ptr, None if blocked is None else blocked.ptr, None,
                C.byref(r) if want_result else None))
            if not want_result:
                return None
            out = {"n_kept": int(r.n_kept), "n_bad_edges": int(r.n_bad_edges), "n_roots": int(r.n_roots)}
            if blocked is not None:
                out["n_blocked"] = int(blocked.download(np.int64, (1,))[0])
            if want_hit:
                n = self.stats()[0]
                out["hit"] = hit.download(np.int64, (self.capacity,))[:n].copy() if hit is not None else np.full(n, -1, np.int64)
            return out
        finally:
            for b in (hit, blocked):
                if b is not None:
                    b.free()

    def find(self, hashes, query=None):
        """Node id of every hash (with query: of every (query, hash) pair; [n] or one for all), -1 for one the table
        does not hold."""
        h = np.ascontiguousarray(hashes, dtype=np.uint64).ravel()
        out = np.full(h.size, -1, np.int32)
        if query is None:
            self._check(_abi.lib().mplx_table_find(self._tab, h.ctypes.data, h.size, out.ctypes.data))
        else:
            q = np.ascontiguousarray(np.broadcast_to(np.asarray(query, dtype=np.int32), (h.size,)))
            self._check(_abi.lib().mplx_table_find_multi(self._tab, h.ctypes.data, q.ctypes.data, h.size, out.ctypes.data))
        return out

    def query_ptr(self):
        """Device address of the per-node query column (None for a table of one query)."""
        p, q = C.c_void_p(), C.c_int32()
        self._check(_abi.lib().mplx_table_query_of(self._tab, C.byref(p), C.byref(q)))
        return p.value

    def path(self, node_id, cap=None):
        """(ids, actions) of the chain of best predecessors from a seed to `node_id`, root first: actions[i] leads from
        ids[i] to ids[i + 1].  With the seed's state (state_of(ids[0])) the actions are a rollout / trajectory."""
        cap = self.stats()[0] if cap is None else int(cap)
        ids = np.zeros(cap + 1, np.int32)
        act = np.zeros(max(cap, 1), np.int32)
        n = C.c_int64(0)
        self._check(_abi.lib().mplx_table_path(self._tab, int(node_id), ids.ctypes.data, act.ctypes.data, cap, C.byref(n)))
        return ids[:n.value + 1].copy(), act[:n.value].copy()

    def view(self):
        v = _abi.TableView()
        self._check(_abi.lib().mplx_table_view_of(self._tab, C.byref(v)))
        return v

    def _read(self, ptr, dtype, count):
        out = np.empty(count, dtype=dtype)
        if count:
            self._check(_abi.lib().mplx_memcpy_d2h(self._env._ctx, out.ctypes.data, int(ptr), out.nbytes))
        return out

    def download(self):
        """The used prefix of every node array: n_nodes, hash, g, pred, pred_action, query (zeros for a table of one
        query), state [4D+2][n_nodes]."""
        n, status = self.stats()
        v = self.view()
        st = np.empty((self.n_fields, n), np.float64)
        for f in range(self.n_fields):
            st[f] = self._read(v.state + 8 * f * v.state_stride, np.float64, n)
        qp = self.query_ptr()
        return {"n_nodes": n, "status": status, "hash": self._read(v.hash, np.uint64, n), "g": self._read(v.g, np.float64, n),
                "query": self._read(qp, np.int32, n) if qp else np.zeros(n, np.int32),
                "pred": self._read(v.pred, np.int32, n), "pred_action": self._read(v.pred_action, np.int32, n), "state": st}

    def state_of(self, node_id):
        """The 4D+2 state row of one node."""
        self.stats()
        v = self.view()
        return np.array([self._read(v.state + 8 * (f * v.state_stride + int(node_id)), np.float64, 1)[0] for f in range(self.n_fields)])
