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
same loop runs Q searches at once: EnvMap.search_many.  opn.set_priors(...) (include/mplx_prior.h) steers every query by
a prior trajectory -- coarse-to-fine planning is two searches, the second with priors=first.as_priors().
env.alloc_field() gives a GoalField (include/mplx_field.h): the grid distance of every cell to a goal region, which
opn.set_field(...) -- search(..., field=True) -- puts under the heuristic so that it sees walls and dead ends.
"""
import contextlib
import ctypes as C
import math

import numpy as np

from . import _abi
from .poly import _conflict_in, _conflict_steps
from .rows import DeviceArray, _device_ptr
from .table import NodeTable, TableFrontier

IS_OPEN, IS_GOAL, SEEN = _abi.OPEN_IS_OPEN, _abi.OPEN_IS_GOAL, _abi.OPEN_SEEN
SELECTED, FOUND, EMPTY = _abi.OPEN_SELECTED, _abi.OPEN_FOUND, _abi.OPEN_EMPTY
# statuses of a SearchResult beyond those of a select: the search stopped at a limit with nodes still open
MAX_ROUNDS, MAX_EXPAND = 3, 4
STATUS_NAMES = {SELECTED: "SELECTED", FOUND: "FOUND", EMPTY: "EMPTY", MAX_ROUNDS: "MAX_ROUNDS", MAX_EXPAND: "MAX_EXPAND"}


class Prior:
    """A prior trajectory and what it was planned with: start row [4D+2], actions [S] (rows of U), the control flag,
    the control table U [nU][udim] and the primitive duration dt of the planner that made it."""

    def __init__(self, start, actions, control, U, dt):
        self.start = np.array(start, dtype=np.float64).ravel()
        self.actions = np.array(actions, dtype=np.int32).ravel()
        self.control = int(control)
        self.U = np.ascontiguousarray(U, dtype=np.float64)
        self.dt = float(dt)

    def __repr__(self):
        return "Prior(%d segments, control=%#x, dt=%r)" % (self.actions.size, self.control, self.dt)


def _prior_of(result, q):
    prm = result._params
    if prm is None or prm.get("U") is None:
        raise RuntimeError("as_prior: the search kept no control table")
    start, act = result.path() if q is None else result.path(q)
    return Prior(start, act, prm["control"], prm["U"], prm["dt"])


def float_to_int(x, origin, res):
    """MapUtil::floatToInt (map_util.h:103-108) of one coordinate: (int)round((x - origin) / res - 0.5), halves away from
    zero as C's round takes them."""
    v = (np.float64(x) - np.float64(origin)) / np.float64(res) - np.float64(0.5)
    if not np.isfinite(v) or abs(v) >= 2.0 ** 31:
        raise ValueError("float_to_int: %r is not a cell of any map" % (x,))
    r = math.floor(v)
    d = v - r  # (exact)
    return int(r + 1 if (d >= 0.5 if v >= 0 else d > 0.5) else r)


class GoalField:
    """mplx_field of an EnvMap (include/mplx_field.h): F goal distance fields over the map's cells.  Build it after the
    map, the search region and the potential map are what the search will see; anything that can change a blocked bit
    afterwards makes it stale, and a push with a stale field is an error.  With a potential map installed a cell blocks at
    a value >= 100; cells of 1 .. 99 cost and are traversable.  Free it (or let it go) before the EnvMap is closed; an open
    set it is still in force in refuses its pushes from then on."""

    def __init__(self, env):
        self._env = env
        self._fld = None
        f = C.c_void_p()
        _abi.check(env._ctx, _abi.lib().mplx_field_create(env._ctx, C.byref(f)))
        self._fld = f

    def _check(self, rc):
        _abi.check(self._env._ctx, rc)

    def build_boxes(self, lo, hi):
        """mplx_field_build: lo, hi [F][D] inclusive seed boxes in cell indices (clipped to the map by the call)."""
        env = self._env
        env._flush()
        lo = np.ascontiguousarray(np.asarray(lo, dtype=np.int32).reshape(-1, env.dim))
        hi = np.ascontiguousarray(np.asarray(hi, dtype=np.int32).reshape(-1, env.dim))
        if lo.shape != hi.shape:
            raise ValueError("build_boxes: lo and hi must both be [F][%d]" % env.dim)
        self._check(_abi.lib().mplx_field_build(self._fld, lo.shape[0], lo.ctypes.data, hi.ctypes.data))
        return self

    def build(self, goal_rows, tol_pos=0.5):
        """One field per goal row ([F][4D+2], or [F][D] positions) with the seed box floatToInt(goal - tol) - 1 ..
        floatToInt(goal + tol) + 1: one cell wider than the goal region on every side, so that no rounding of goal -+ tol
        leaves a goal-region cell unseeded (extra seeds only lower dist).  tol_pos: one value or [F]."""
        env = self._env
        if env._geometry is None:
            raise RuntimeError("GoalField.build: set the map first")
        _, origin, res = env._geometry
        rows = np.atleast_2d(np.asarray(goal_rows, dtype=np.float64))
        tol = np.broadcast_to(np.asarray(tol_pos, dtype=np.float64), (rows.shape[0],))
        lo = [[float_to_int(rows[f, i] - tol[f], origin[i], res) - 1 for i in range(env.dim)] for f in range(rows.shape[0])]
        hi = [[float_to_int(rows[f, i] + tol[f], origin[i], res) + 1 for i in range(env.dim)] for f in range(rows.shape[0])]
        return self.build_boxes(lo, hi)

    @property
    def shape(self):
        """(F, n_cells); (0, 0) while the field is empty."""
        F, n = C.c_int32(), C.c_int64()
        self._check(_abi.lib().mplx_field_shape(self._fld, C.byref(F), C.byref(n)))
        return int(F.value), int(n.value)

    @property
    def F(self):
        return self.shape[0]

    @property
    def stale(self):
        return _abi.lib().mplx_field_is_stale(self._fld) == 1

    @property
    def passes(self):
        """Passes of the last build (diagnostic: part of no result)."""
        n = C.c_int64()
        self._check(_abi.lib().mplx_field_passes(self._fld, C.byref(n)))
        return int(n.value)

    def view(self):
        v = _abi.FieldView()
        self._check(_abi.lib().mplx_field_view_of(self._fld, C.byref(v)))
        return v

    def dist(self):
        """A download: int32 [F][n_cells], cell index as MapUtil::getIndex."""
        F, n = self.shape
        out = np.empty((F, n), np.int32)
        if F:
            self._check(_abi.lib().mplx_field_download(self._fld, out.ctypes.data))
        return out

    def free(self):
        if self._fld and self._env._ctx:
            _abi.lib().mplx_field_destroy(self._fld)
        self._fld = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _distinct_goals(goal_rows, tol_pos):
    """(rows [F][.], tol [F], field_of_query [Q]): one entry per distinct (goal row, tol_pos), in order of appearance."""
    rows = np.atleast_2d(np.asarray(goal_rows, dtype=np.float64))
    tol = np.broadcast_to(np.asarray(tol_pos, dtype=np.float64), (rows.shape[0],))
    seen, foq, keep = {}, [], []
    for q in range(rows.shape[0]):
        key = (rows[q].tobytes(), float(tol[q]))
        if key not in seen:
            seen[key] = len(keep)
            keep.append(q)
        foq.append(seen[key])
    return rows[keep], tol[keep], np.array(foq, np.int32)


def _field_setup(who, env, opn, field, field_of_query, goal_rows, tol_pos, prior):
    """The `field` argument of a search, after the goals are set: (field, owned, field_of_query)."""
    if field is None or field is False:
        return None, False, None
    if prior is not None:
        raise ValueError("%s: field and prior(s) exclude each other" % who)
    owned = field is True
    if owned:
        rows, tol, field_of_query = _distinct_goals(goal_rows, tol_pos)
        field = GoalField(env)
    try:
        if owned:
            field.build(rows, tol)
        opn.set_field(field, field_of_query)
    except Exception:
        if owned:
            field.free()
        raise
    foq = None if field_of_query is None else np.array(field_of_query, np.int32).ravel()
    return field, owned, foq


class OpenSet:
    """mplx_open of a NodeTable.  Free it (or let it go) before the table."""

    def __init__(self, env, table):
        self._env = env
        self._table = table  # (kept alive: the open set reads the table's arrays)
        self._open = None
        self._field = None  # (kept alive while it is in force)
        self.has_priors, self.heur_mode = False, None  # what is in force, as the calls below left it (bound() asks)
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

    def push(self, frontier, n_max=None, eps=1.0, sight=False, closed=False):
        """mplx_open_push_device: the first min(count on the device, n_max, capacity) rows of `frontier` become open
        with f = g + eps * h.  closed: mplx_open_push_closed_device (include/mplx_replan.h) -- key and goal bit are
        set, the nodes stay closed.  Asynchronous."""
        f = frontier.c_struct()
        n = frontier.capacity if n_max is None else int(n_max)
        fn = _abi.lib().mplx_open_push_closed_device if closed else _abi.lib().mplx_open_push_device
        self._check(fn(self._open, C.byref(f), n, float(eps), 1 if sight else 0))

    def select(self, delta, frontier, want_result=True, d_result=None, best=None):
        """mplx_open_select_device into `frontier`.  Returns the result as a dict (one synchronisation), or None with
        want_result=False -- the call is then asynchronous; d_result: a device buffer of 48 bytes, or None.
        best=k: mplx_open_select_best_device (include/mplx_best.h) -- of the open nodes with f <= f_min + delta only
        the k smallest keys (ties by id) are selected.  It changes what a round expands, never when the goal is
        announced: the stopping rule is the plain select's."""
        f = frontier.c_struct()
        r = _abi.OpenResult()
        d_res, h_res = d_result.ptr if d_result is not None else None, C.byref(r) if want_result else None
        if best is None:
            self._check(_abi.lib().mplx_open_select_device(self._open, float(delta), C.byref(f), d_res, h_res))
        else:
            self._check(_abi.lib().mplx_open_select_best_device(self._open, int(best), float(delta), C.byref(f), d_res, h_res))
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
        gcs = np.broadcast_to(np.asarray(goal_control, dtype=np.int64), (n,))  # (one flag for all queries, or [Q])
        specs = (_abi.GoalSpec * max(n, 1))()
        for q in range(n):
            g = specs[q]
            g.goal, g.control, g.goal_control = rows[q].ctypes.data, int(env._p.control), int(gcs[q])
            g.w, g.v_max = float(ws[q]), float(vs[q])
            g.tol_pos, g.tol_vel, g.tol_acc, g.tol_yaw = float(tp[q]), float(tv[q]), float(ta[q]), float(ty[q])
        self._check(_abi.lib().mplx_open_set_goals(self._open, specs, n))
        self._field = None  # (dropped by the call)
        self.has_priors = False  # (likewise)

    def select_many(self, delta, frontier, want_result=True, d_results=None, best=None):
        """mplx_open_select_multi_device into `frontier`.  Returns the Q results as a list of dicts (one
        synchronisation), or None with want_result=False; d_results: a device buffer of Q * 48 bytes, or None.
        best=k: mplx_open_select_best_multi_device (include/mplx_best.h) -- per query the k smallest keys among its
        open nodes with f <= f_min + delta; the stopping rule of every query is unchanged."""
        f = frontier.c_struct()
        res = (_abi.OpenResult * self.n_queries)()
        d_res, h_res = d_results.ptr if d_results is not None else None, res if want_result else None
        if best is None:
            self._check(_abi.lib().mplx_open_select_multi_device(self._open, float(delta), C.byref(f), d_res, h_res))
        else:
            self._check(_abi.lib().mplx_open_select_best_multi_device(self._open, int(best), float(delta), C.byref(f), d_res, h_res))
        if not want_result:
            return None
        return [{"status": int(r.status), "goal_id": int(r.goal_id), "count": int(r.count), "n_open": int(r.n_open),
                 "f_min": float(r.f_min), "goal_f": float(r.goal_f), "goal_g": float(r.goal_g)} for r in res]

    def set_priors(self, starts, actions, control, U, dt):
        """mplx_open_set_priors_device: starts [4D+2][Q] (or one state for all), actions [H][Q] (-1 ends; a first action
        of -1: no prior for that query), and the source the priors were planned with (control flag, control table U
        [nU][udim], primitive duration dt).  Replaces the priors of all queries; needs set_goals first.  Returns
        {"status" [Q] (TRAJ_* bits), "n_steps" [Q]} (one synchronisation)."""
        env = self._env
        env._flush()
        s, keep, K, H = env._traj_host_set(starts, actions)
        starts_h, actions_h = keep
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.ndim != 2:
            raise ValueError("U must be [nU][udim]")
        bufs = [DeviceArray(env, max(a.nbytes, 8)) for a in (starts_h, actions_h, U)]
        try:
            for b, a in zip(bufs, (starts_h, actions_h, U)):
                if a.nbytes:
                    b.upload(a)
            s.starts, s.actions = bufs[0].ptr, bufs[1].ptr
            src = _abi.PriorSource()
            src.control, src.nU, src.udim, src.U, src.dt = int(control), U.shape[0], U.shape[1], bufs[2].ptr, float(dt)
            status, n_steps = np.zeros(max(K, 1), np.uint8), np.zeros(max(K, 1), np.int32)
            info = _abi.PriorInfo()
            info.status, info.n_steps = status.ctypes.data, n_steps.ctypes.data
            # (the info read-back synchronises: the uploads may be freed when the call returns)
            self.has_priors = False  # (a failure leaves the open set without priors)
            self._check(_abi.lib().mplx_open_set_priors_device(self._open, C.byref(src), C.byref(s), C.byref(info)))
            self.has_priors = True
        finally:
            for b in bufs:
                b.free()
        return {"status": status[:K], "n_steps": n_steps[:K]}

    def set_prior_list(self, priors):
        """set_priors from [Q] Prior or None entries; the priors of one call share control flag, U and dt."""
        env = self._env
        some = [p for p in priors if p is not None]
        if len(priors) != self.n_queries:
            raise ValueError("priors: %d entries for %d queries" % (len(priors), self.n_queries))
        if not some:
            self.clear_priors()
            return None
        p0 = some[0]
        for p in some[1:]:
            if p.control != p0.control or p.dt != p0.dt or p.U.shape != p0.U.shape or not np.array_equal(p.U, p0.U):
                raise ValueError("priors: the priors of one call must share control flag, control table and dt")
        H = max(1, max(p.actions.size for p in some))
        starts = np.zeros((env.n_fields, len(priors)))
        actions = np.full((H, len(priors)), -1, np.int32)
        for q, p in enumerate(priors):
            if p is not None:
                starts[:, q] = p.start
                actions[:p.actions.size, q] = p.actions
        return self.set_priors(starts, actions, p0.control, p0.U, p0.dt)

    def clear_priors(self):
        self._check(_abi.lib().mplx_open_clear_priors(self._open))
        self.has_priors = False

    def set_field(self, field, field_of_query=None):
        """mplx_open_set_field: every push takes the heuristic of query q from field field_of_query[q] of `field` (a
        GoalField); None: query q uses field q; -1: that query keeps the default heuristic.  In force until clear_field or
        set_goals; clear() leaves it."""
        self._env._flush()
        foq = None
        if field_of_query is not None:
            foq = np.ascontiguousarray(field_of_query, dtype=np.int32).ravel()
            if foq.size != self.n_queries:
                raise ValueError("field_of_query: %d entries for %d queries" % (foq.size, self.n_queries))
        self._check(_abi.lib().mplx_open_set_field(self._open, field._fld, None if foq is None else foq.ctypes.data))
        self._field = field

    def clear_field(self):
        self._check(_abi.lib().mplx_open_clear_field(self._open))
        self._field = None

    def set_heur(self, mode):
        """mplx_open_set_heur (include/mplx_heur.h): "robust" -- every push from now on takes its heuristic from the
        dynamics-aware ROBUST form (never below the default; with a field the larger of the two); None / "default" -- the
        default again.  clear() keeps the mode; priors exclude it."""
        m = _abi.heur_mode(mode)
        self._check(_abi.lib().mplx_open_set_heur(self._open, m))
        self.heur_mode = None if m == _abi.HEUR_DEFAULT else "robust"

    def rekey(self, eps, cut=None, write=True, want_result=True, d_bound=None):
        """mplx_open_rekey_device (include/mplx_anytime.h): every node of the table that was ever pushed gets the key
        g + eps * h again, with the table's current g and the h a push would compute now; per query the smallest g + h
        among its open nodes is reported.  cut: one value or [Q] -- an open node of query q with g + h >= cut[q] is closed
        (ties too; inf closes nothing); write=False: the bound alone, no byte of f or flags changes.  Returns the Q
        bounds as a list of dicts {"lower", "n_open", "n_pruned", "n_rekeyed"} (one synchronisation), or None with
        want_result=False; d_bound: a device buffer of Q * 32 bytes, or None.  Without cut and result the call is
        asynchronous."""
        Q = self.n_queries
        res = (_abi.OpenBound * Q)()
        h_cut = None
        if cut is not None:
            self._env._flush()
            h_cut = np.ascontiguousarray(np.broadcast_to(np.asarray(cut, dtype=np.float64), (Q,)))
        self._check(_abi.lib().mplx_open_rekey_device(self._open, float(eps), 1 if write else 0,
                                                      None if h_cut is None else h_cut.ctypes.data,
                                                      d_bound.ptr if d_bound is not None else None, res if want_result else None))
        if not want_result:
            return None
        return [{"lower": float(r.lower), "n_open": int(r.n_open), "n_pruned": int(r.n_pruned), "n_rekeyed": int(r.n_rekeyed)}
                for r in res]

    def priors(self):
        """The prior table in force (a download): {"n_steps" [Q], "pos": [Q] arrays [n_steps][D], "togo": [Q] arrays,
        "goal_row" [Q][4D+2], "goal_hash" [Q]}, or None while no prior is in force."""
        v = _abi.PriorView()
        self._check(_abi.lib().mplx_open_prior_view_of(self._open, C.byref(v)))
        if not v.n_steps:
            return None
        Q, K, D, rd = self.n_queries, int(v.step_capacity), self._env.dim, self._table._read
        n = rd(v.n_steps, np.int32, Q)
        pos, togo = rd(v.pos, np.float64, Q * K * D).reshape(Q, K, D), rd(v.togo, np.float64, Q * K).reshape(Q, K)
        return {"n_steps": n, "pos": [pos[q, :n[q]].copy() for q in range(Q)], "togo": [togo[q, :n[q]].copy() for q in range(Q)],
                "goal_row": rd(v.goal_row, np.float64, Q * 14).reshape(Q, 14)[:, :self._env.n_fields].copy(),
                "goal_hash": rd(v.goal_hash, np.uint64, Q)}

    def view(self):
        v = _abi.OpenView()
        self._check(_abi.lib().mplx_open_view_of(self._open, C.byref(v)))
        return v

    def download(self):
        """f and flags of the table's nodes: {"n_nodes", "f", "flags"}; f is meaningful where flags has SEEN."""
        n = self._table.stats()[0]
        v = self.view()
        return {"n_nodes": n, "f": self._table._read(v.f, np.float64, n), "flags": self._table._read(v.flags, np.uint8, n)}


def _smooth(env, paths, v, control):
    """The paths [(start, actions) or None] of Q queries -> chain states on the device (mplx_traj_info_device, want_states)
    -> one mplx_solve_device for Q x n_v problems, problem vi * Q + q = path q at speed v[vi]; the states never visit the
    host.  A query without a path is an empty problem (SOLVE_EMPTY)."""
    env._flush()
    vs = np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel()
    Q, nv = len(paths), len(vs)
    K = Q * nv
    H = max([len(p[1]) for p in paths if p is not None] + [1])
    starts = np.zeros((env.n_fields, K))
    actions = np.full((H, K), -1, np.int32)
    n_wp = np.zeros(K, np.int32)
    for q, p in enumerate(paths):
        if p is None:
            continue
        for vi in range(nv):
            k = vi * Q + q
            starts[:, k] = p[0]
            actions[:len(p[1]), k] = p[1]
            n_wp[k] = len(p[1]) + 1
    bufs = [DeviceArray(env, a.nbytes) for a in (starts, actions, n_wp, np.zeros(K))]
    info = poly = None
    try:
        for b, a in zip(bufs, (starts, actions, n_wp, np.repeat(vs, Q))):
            b.upload(a)
        info = env.alloc_traj_info(K, H, want_states=True)
        env.traj_info_resident(bufs[0], bufs[1], info, H)
        poly = env.alloc_poly(K, H + 1)
        out = env.alloc_solve_out(K, H + 1, control)
        try:
            env.solve_traj_resident(poly, info.seg_state, K, H + 1, n_wp=bufs[2], v_arr=bufs[3], control=control, out=out)
        except Exception:
            out.free()
            raise
        env.synchronize()
        return poly
    except Exception:
        if poly is not None:
            poly.free()
        raise
    finally:
        for b in bufs:
            b.free()
        if info is not None:
            info.free()


def _smooth_timed(env, paths, control, avoid, t0, radius, ignore_group):
    """smooth(timed=True): one solve per path with dts = the differences of the chain states' own t row (the dts path
    EnvMap.connect uses; repeated waypoints, as wait edges leave them, are legal there), so the polynomial passes every
    chain state at the chain's own time.  The t row is read back, differenced on the host and uploaded.  With avoid: a
    Reservations.check_poly of the result with the robots' t0 / radius / ignore_group; its dict is poly.reserve_hit."""
    env._flush()
    Q = len(paths)
    H = max([len(p[1]) for p in paths if p is not None] + [1])
    starts = np.zeros((env.n_fields, Q))
    actions = np.full((H, Q), -1, np.int32)
    n_wp = np.zeros(Q, np.int32)
    for q, p in enumerate(paths):
        if p is not None:
            starts[:, q] = p[0]
            actions[:len(p[1]), q] = p[1]
            n_wp[q] = len(p[1]) + 1
    bufs = [DeviceArray(env, a.nbytes) for a in (starts, actions, n_wp, np.zeros((H, Q)))]
    info = poly = None
    try:
        for b, a in zip(bufs[:3], (starts, actions, n_wp)):
            b.upload(a)
        info = env.alloc_traj_info(Q, H, want_states=True)
        env.traj_info_resident(bufs[0], bufs[1], info, H)
        env.synchronize()
        t = info.seg_state.download(np.float64, (H + 1, Q), offset=(env.n_fields - 1) * (H + 1) * Q * 8)
        dts = np.where(np.arange(H)[:, None] + 1 < n_wp[None, :], t[1:] - t[:-1], 0.0)
        bufs[3].upload(dts)
        poly = env.alloc_poly(Q, H + 1)
        out = env.alloc_solve_out(Q, H + 1, control)
        try:
            env.solve_traj_resident(poly, info.seg_state, Q, H + 1, n_wp=bufs[2], dts=bufs[3], control=control, out=out)
        except Exception:
            out.free()
            raise
        env.synchronize()
        poly.chain_times, poly.reserve_hit = t, None
        if avoid is not None:
            poly.reserve_hit = avoid.check_poly(poly, t0, radius, ignore_group)
        return poly
    except Exception:
        if poly is not None:
            poly.free()
        raise
    finally:
        for b in bufs:
            b.free()
        if info is not None:
            info.free()


def _shortcut(env, paths, max_hop, control, avoid=None, t0=None, radius=None, ignore_group=None):
    """The paths [(start, actions) or None] of Q queries -> chain states on the device (mplx_traj_info_device, want_states)
    -> mplx_shortcut_device (with avoid: mplx_shortcut_timed_device); only counts, costs and statuses are read back.  A
    query without a path is an empty problem."""
    env._flush()
    Q = len(paths)
    H = max([len(p[1]) for p in paths if p is not None] + [1])
    starts = np.zeros((env.n_fields, Q))
    actions = np.full((H, Q), -1, np.int32)
    n_wp = np.zeros(Q, np.int32)
    for q, p in enumerate(paths):
        if p is not None:
            starts[:, q] = p[0]
            actions[:len(p[1]), q] = p[1]
            n_wp[q] = len(p[1]) + 1
    bufs = [DeviceArray(env, a.nbytes) for a in (starts, actions, n_wp)]
    info = None
    try:
        for b, a in zip(bufs, (starts, actions, n_wp)):
            b.upload(a)
        info = env.alloc_traj_info(Q, H, want_states=True)
        env.traj_info_resident(bufs[0], bufs[1], info, H)
        return env.shortcut_resident(info.seg_state, Q, H + 1, n_wp=bufs[2], control=control, max_hop=max_hop, avoid=avoid, t0=t0,
                                     radius=radius, ignore_group=ignore_group)
    finally:
        for b in bufs:
            b.free()
        if info is not None:
            info.free()


def pick_fastest(poly, Q, vs, v_max=None, a_max=None, j_max=None):
    """Of the Q x n_v candidates smooth(v=vs) returned (problem vi * Q + q = path q at speed vs[vi]), per query the index
    vi of the largest speed whose candidate was solved (status 0), is valid under PolyTrajSet.limits(all_roots=True)
    with the given limits (default: the EnvMap's) and has a finite traverse cost on the map as it is now; -1 where no
    candidate passes.  Returns an int array [Q]."""
    vs = np.atleast_1d(np.asarray(vs, dtype=np.float64)).ravel()
    Q = int(Q)
    if poly.n != Q * len(vs):
        raise ValueError("pick_fastest: the set holds %d problems, not Q x n_v = %d" % (poly.n, Q * len(vs)))
    lim = poly.limits(v_max=v_max, a_max=a_max, j_max=j_max, all_roots=True)
    trav = poly.traverse()
    good = ((poly.status == 0) & (lim["valid"] == 1) & (trav["status"] == 0) & np.isfinite(trav["cost"])).reshape(len(vs), Q)
    speed = np.where(good, vs[:, None], -np.inf)
    best = np.argmax(speed, axis=0)
    return np.where(good.any(axis=0), best, -1).astype(np.int64)


def _path_set(env, paths):
    """The paths [(start, actions) or None] of Q queries as one trajectory set: starts [4D+2][Q], actions [H][Q]; a query
    without a path is an empty chain (TRAJ_EMPTY)."""
    Q = len(paths)
    H = max([len(p[1]) for p in paths if p is not None] + [1])
    starts = np.zeros((env.n_fields, Q))
    actions = np.full((H, Q), -1, np.int32)
    for q, p in enumerate(paths):
        if p is not None:
            starts[:, q] = p[0]
            actions[:len(p[1]), q] = p[1]
    return starts, actions


def stagger(trajs, step, radius, rank=None, delay=None, max_rounds=64, park=False, group=None, t0=None):
    """Prioritised delaying on top of conflicts(): trajs is anything with conflicts(step, t0=, radius=, group=, rank=,
    park=) -- a PolyTrajSet, a MultiSearchResult.  Each round makes one conflicts call with `rank` (default: the index,
    so trajectory 0 never yields) and adds `delay` (default 4 * step) to t0 of every trajectory with a conflict charged to
    it; it stops when none is charged, or after max_rounds rounds.  Returns (t0 [K], resolved [K] bool -- no conflict
    was charged in the last call made --, rounds = the calls made); t0 holds the delays added after that last call too.

    Its limits: it only ever delays, along paths it does not change.  Under park=True a robot that waits -- at its start
    or at its end -- in the way of a robot of higher priority is never resolved by delaying it, and is reported
    unresolved at max_rounds; with park=False a robot does not exist outside its own trajectory, which resolves on
    paper what a real robot standing at its goal would not.  Equal ranks are both charged and both delayed: they move
    in lockstep and stay in conflict.  It is a helper on top of the kernel, not a multi-agent planner."""
    K = _n_traj(trajs) if t0 is None else np.size(t0)
    t = np.zeros(K) if t0 is None else np.array(t0, dtype=np.float64).ravel()
    rank = np.arange(K, dtype=np.int32) if rank is None else np.asarray(rank, dtype=np.int32)
    add = 4.0 * float(step) if delay is None else float(delay)
    charged, rounds = np.zeros(K, dtype=bool), 0
    for _ in range(int(max_rounds)):
        res = trajs.conflicts(step, t0=t, radius=radius, group=group, rank=rank, park=park)
        rounds += 1
        charged = res.first_step >= 0
        if not charged.any():
            break
        t = np.where(charged, t + add, t)
    return t, ~charged, rounds


def _n_traj(trajs):
    return int(trajs.n_queries if hasattr(trajs, "n_queries") else trajs.n)


def _unpack_hits(hit, status, n_hit):
    """The dict Reservations.check_poly returns: instant and partner unpacked from hit, -1 where hit < 0."""
    some = hit >= 0
    return {"hit": hit, "instant": np.where(some, hit >> 32, -1).astype(np.int32),
            "partner": np.where(some, hit & 0xffffffff, -1).astype(np.int32), "status": status, "n_hit": n_hit}


class Reservations:
    """mplx_reserve of an EnvMap's context (include/mplx_reserve.h): the positions of B reserved trajectories at the
    instants i * step of a common clock, kept on the device, and the check of successor lists against them.  trajs: a
    PolyTrajSet, or (starts, actions) chains as EnvMap.traj_conflicts takes them; t0 / radius / group / park as
    conflicts() takes them.  The `avoid` of EnvMap.search / search_many.  free() it before the EnvMap is closed."""

    def __init__(self, env, trajs, step, n_steps=None, t0=None, radius=None, group=None, park=True):
        self._env, self._res = env, None
        self._q = None
        r = C.c_void_p()
        _abi.check(env._ctx, _abi.lib().mplx_reserve_create(env._ctx, C.byref(r)))
        self._res = r
        try:
            self.fill(trajs, step, n_steps, t0, radius, group, park)
        except Exception:
            self.free()
            raise

    def _check(self, rc):
        _abi.check(self._env._ctx, rc)

    def fill(self, trajs, step, n_steps=None, t0=None, radius=None, group=None, park=True):
        """Fills the table again (mplx_reserve_fill_poly / _fill_traj; synchronous).  n_steps=None: the smallest count
        whose instants cover max(t0 + total), as conflicts() takes it."""
        env = self._env
        env._flush()
        if hasattr(trajs, "_h"):  # a PolyTrajSet
            trajs._need()
            K = trajs.n
            if n_steps is None:
                inf = trajs.info()
                n_steps = _conflict_steps(float(step), t0, inf["total_time"], inf["status"] == 0)
            i, keep = _conflict_in(K, step, n_steps, t0, radius, group, None, park, 0, False)
            self._check(_abi.lib().mplx_reserve_fill_poly(self._res, trajs._h, C.byref(i)))
        else:
            starts, actions = trajs
            s, keep2, K, H = env._traj_host_set(starts, actions)
            if n_steps is None:
                inf = env.traj_info(starts, actions) if K else {"total_time": np.zeros(0), "status": np.zeros(0, np.uint8)}
                n_steps = _conflict_steps(float(step), t0, inf["total_time"], inf["status"] == 0)
            i, keep = _conflict_in(K, step, n_steps, t0, radius, group, None, park, 0, False)
            self._check(_abi.lib().mplx_reserve_fill_traj(self._res, env._ctx, C.byref(s), C.byref(i)))
        self.n, self.n_steps, self.step = int(K), int(n_steps), float(step)

    def set_queries(self, t0, radius, ignore_group=None):
        """mplx_reserve_set_queries: per planning robot its start on the clock, its radius and the group whose
        reservations it ignores (-1 / None: none); [Q] each, or scalars for one query."""
        t0 = np.ascontiguousarray(np.atleast_1d(np.asarray(t0, dtype=np.float64)))
        Q = t0.size
        rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (Q,)))
        ign = None if ignore_group is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ignore_group, dtype=np.int32), (Q,)))
        self._check(_abi.lib().mplx_reserve_set_queries(self._res, Q, t0.ctypes.data, rad.ctypes.data,
                                                        None if ign is None else ign.ctypes.data))
        self.n_queries = Q

    def check(self, frontier, lists, n, table=None, hit=None, n_blocked=None):
        """mplx_reserve_check_device on the lists the expansion of `frontier` (its first n rows) left: the entries that
        come too close to a reservation get cost +inf.  table: the NodeTable whose query column says whose a row is
        (needed with more than one query).  hit: a device buffer of lists.n_slots int64, n_blocked: one of 8 bytes that
        the call adds to; either may be None.  Asynchronous."""
        s = lists.c_struct()
        self._check(_abi.lib().mplx_reserve_check_device(
            self._res, None if table is None else table._tab, C.byref(s), int(n), _device_ptr(frontier.id), int(frontier.ptr),
            int(frontier.n_nodes), None if hit is None else _device_ptr(hit), None if n_blocked is None else _device_ptr(n_blocked)))

    def add_waits(self, frontier, lists, n, n_added=None):
        """mplx_lists_add_wait_device (include/mplx_wait.h) on the lists the expansion of `frontier` (its first n rows)
        left, before check(): every row whose parent stands still under the all-zero control gets that control's entry,
        the last of its list -- "wait for one primitive", which the expansion drops.  n_added: a device buffer of 8
        bytes that the call adds to, or None.  The call reads nothing of the reservation table; it lives here because a
        wait is only worth an edge among reservations.  A `zero_rows` mask of `lists` stays valid.  Asynchronous."""
        s = lists.c_struct()
        self._check(_abi.lib().mplx_lists_add_wait_device(
            self._env._ctx, C.byref(s), int(n), int(frontier.ptr), int(frontier.n_nodes), _device_ptr(frontier.id),
            None if n_added is None else _device_ptr(n_added)))

    def park(self, open_set, frontier, n_max, hit=None, n_vetoed=None):
        """mplx_reserve_park_device right after open_set.push(frontier, n_max): a goal-region node at which the robot
        could not stay -- a reservation comes too close at some instant from the node's t on -- loses IS_GOAL and stays
        an ordinary open node.  hit: a device buffer of frontier.capacity int64, n_vetoed: one of 8 bytes that the call
        adds to; either may be None.  Asynchronous."""
        f = frontier.c_struct()
        self._check(_abi.lib().mplx_reserve_park_device(
            self._res, open_set._open, C.byref(f), int(n_max), None if hit is None else _device_ptr(hit),
            None if n_vetoed is None else _device_ptr(n_vetoed)))

    def check_poly(self, poly, t_start, radius=None, ignore_group=None):
        """mplx_reserve_check_poly (include/mplx_reserve_poly.h; synchronous): the K trajectories of the PolyTrajSet
        `poly`, trajectory k starting at t_start[k] on the table's clock, against the reservations.  t_start [K] or a
        scalar (finite, may be negative), radius [K] or a scalar (None: 0), ignore_group [K], a scalar or None (-1).
        Returns {"hit" [K] int64: the smallest (instant << 32 | reservation) in conflict, -1 none, -2 the trajectory
        leaves the table's horizon; "instant", "partner" [K] int32 unpacked from it, -1 where there is none; "status"
        [K]: the set's status bits | CONFLICT_BAD_INPUT; "n_hit": the problems with hit != -1}."""
        self._env._flush()
        poly._need()
        K = int(poly.n)
        ts = np.ascontiguousarray(np.broadcast_to(np.asarray(t_start, dtype=np.float64), (K,)))
        i, o = _abi.ReservePolyIn(), _abi.ReservePolyOut()
        i.t_start = ts.ctypes.data
        keep = [ts]
        if radius is None or np.ndim(radius) == 0:
            i.radius_all = 0.0 if radius is None else float(radius)
        else:
            keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float64), (K,))))
            i.radius = keep[-1].ctypes.data
        if ignore_group is not None:
            keep.append(np.ascontiguousarray(np.broadcast_to(np.asarray(ignore_group, dtype=np.int32), (K,))))
            i.ignore_group = keep[-1].ctypes.data
        hit, status, n_hit = np.full(K, -1, np.int64), np.zeros(K, np.uint8), np.zeros(1, np.int64)
        o.hit, o.status, o.n_hit = hit.ctypes.data, status.ctypes.data, n_hit.ctypes.data
        self._check(_abi.lib().mplx_reserve_check_poly(self._res, poly._h, C.byref(i), C.byref(o)))
        return _unpack_hits(hit, status, int(n_hit[0]))

    def check_poly_resident(self, poly, t_start, radius=None, ignore_group=None, hit=None, status=None, n_hit=None):
        """mplx_reserve_check_poly_device: asynchronous, on device buffers.  t_start: [K] doubles; radius: [K] doubles, a
        host scalar or None (0); ignore_group: [K] int32 or None; hit [K] int64, status [K] bytes, n_hit 8 bytes that the
        call adds to; each output may be None."""
        i, o = _abi.ReservePolyIn(), _abi.ReservePolyOut()
        i.t_start = _device_ptr(t_start)
        if radius is None or np.ndim(radius) == 0 and not hasattr(radius, "ptr") and not hasattr(radius, "data_ptr"):
            i.radius_all = 0.0 if radius is None else float(radius)
        else:
            i.radius = _device_ptr(radius)
        if ignore_group is not None:
            i.ignore_group = _device_ptr(ignore_group)
        for key, v in (("hit", hit), ("status", status), ("n_hit", n_hit)):
            if v is not None:
                setattr(o, key, _device_ptr(v))
        self._check(_abi.lib().mplx_reserve_check_poly_device(self._res, poly._h, C.byref(i), C.byref(o)))

    def positions(self):
        """The table (a download, for tests): {"pos" [n_steps][D][B], "active" [n_steps][B], "included" [B], "radius"
        [B], "group" [B], "status" [B]}."""
        B, n, D = self.n, self.n_steps, self._env.dim
        out = {"pos": np.zeros((n, D, B)), "active": np.zeros((n, B), np.uint8), "included": np.zeros(B, np.uint8),
               "radius": np.zeros(B), "group": np.zeros(B, np.int32), "status": np.zeros(B, np.uint8)}
        self._check(_abi.lib().mplx_reserve_positions(self._res, *[out[k].ctypes.data for k in
                                                                   ("pos", "active", "included", "radius", "group", "status")]))
        return out

    def free(self):
        res = self._res
        self._res = None
        if res and self._env._ctx:
            _abi.lib().mplx_reserve_destroy(res)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Body:
    """mplx_body of an EnvMap's context (include/mplx_body.h; EnvMap.alloc_body): the robot as an ellipsoid of radius r
    across the thrust axis and half-height h along it, whose axis follows acc + g e_z, and an obstacle point cloud
    binned on the device; the check of successor lists and of trajectory sets against it.  tilt_max: the largest tilt
    in radians, in (0, pi / 2] (None: pi / 2 -- only a thrust that points down or vanishes is a bad attitude); its
    cosine is taken here, once.  The `body` of EnvMap.search / search_many.  free() it before the EnvMap is closed."""

    def __init__(self, env, r, h, g=9.81, tilt_max=None):
        self._env, self._body = env, None
        b = C.c_void_p()
        _abi.check(env._ctx, _abi.lib().mplx_body_create(env._ctx, C.byref(b)))
        self._body = b
        try:
            self.set_shape(r, h, g, tilt_max)
        except Exception:
            self.free()
            raise

    def _check(self, rc):
        _abi.check(self._env._ctx, rc)

    def set_shape(self, r, h, g=9.81, tilt_max=None, min_cos_tilt=None):
        """mplx_body_set_shape; min_cos_tilt: the cosine itself instead of tilt_max (tests give representable values).  A
        cloud that is in place is kept and binned again."""
        if min_cos_tilt is None:
            min_cos_tilt = 0.0 if tilt_max is None else max(0.0, math.cos(float(tilt_max)))
        self._check(_abi.lib().mplx_body_set_shape(self._body, float(r), float(h), float(g), float(min_cos_tilt)))
        self.r, self.h, self.g, self.min_cos_tilt = float(r), float(h), float(g), float(min_cos_tilt)

    def fill(self, points):
        """mplx_body_fill: points [n][D] (host; synchronous).  A point with a coordinate that is not finite never hits."""
        self._env._flush()
        pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, self._env.dim))
        self._check(_abi.lib().mplx_body_fill(self._body, pts.ctypes.data if len(pts) else None, len(pts)))

    def fill_resident(self, ptr, n):
        """mplx_body_fill_device: n points [n][D] in device memory (a buffer or an address).  Asynchronous."""
        self._env._flush()
        self._check(_abi.lib().mplx_body_fill_device(self._body, _device_ptr(ptr) if n else None, int(n)))

    def fill_map(self, kind=_abi.CELL_OCCUPIED):
        """mplx_body_fill_map: the cells of class `kind` of the map the EnvMap holds now, numbered as EnvMap's voxel
        cloud of that class; the points stay on the device."""
        self._env._flush()
        self._check(_abi.lib().mplx_body_fill_map(self._body, int(kind)))

    def shape(self):
        """{"n", "n_excluded", "cells" [3], "edge", "origin" [3], "generation"} (mplx_body_shape; synchronises)."""
        n, ne, gen, edge = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        cells, origin = np.zeros(3, np.int32), np.zeros(3)
        self._check(_abi.lib().mplx_body_shape(self._body, C.byref(n), C.byref(ne), cells.ctypes.data, C.byref(edge),
                                               origin.ctypes.data, C.byref(gen)))
        return {"n": n.value, "n_excluded": ne.value, "cells": cells, "edge": edge.value, "origin": origin,
                "generation": gen.value}

    @property
    def generation(self):
        return self.shape()["generation"]

    def cells(self):
        """(cell_of_point [n] int32, -1 excluded; cell_start [cells + 1] int32): the binning, a download for tests."""
        sh = self.shape()
        cop, start = np.zeros(sh["n"], np.int32), np.zeros(int(np.prod(sh["cells"].astype(np.int64))) + 1, np.int32)
        self._check(_abi.lib().mplx_body_cells(self._body, cop.ctypes.data if len(cop) else None, start.ctypes.data))
        return cop, start

    def check(self, frontier, lists, n, n_samp=4, hit=None, n_blocked=None):
        """mplx_body_check_device on the lists the expansion of `frontier` (its first n rows) left: the entries along
        which the body touches a point of the cloud at one of n_samp + 1 samples, or has a bad attitude there, get cost
        +inf.  hit: a device buffer of lists.n_slots int64, n_blocked: one of 8 bytes that the call adds to; either may
        be None.  Asynchronous."""
        s = lists.c_struct()
        self._check(_abi.lib().mplx_body_check_device(
            self._body, C.byref(s), int(n), _device_ptr(frontier.id), int(frontier.ptr), int(frontier.n_nodes), int(n_samp),
            None if hit is None else _device_ptr(hit), None if n_blocked is None else _device_ptr(n_blocked)))

    def check_poly(self, poly, step):
        """mplx_body_check_poly (synchronous): the K trajectories of the PolyTrajSet `poly` at the local times i * step
        and at their ends.  Returns {"hit" [K] int64: the smallest (sample << 32 | point), (sample << 32 | 0x7fffffff)
        for a bad attitude, -1 none; "sample", "point" [K] int32 unpacked from it, -1 where there is none; "status" [K]:
        the set's status bits; "n_hit"}."""
        self._env._flush()
        poly._need()
        K = int(poly.n)
        i, o = _abi.BodyPolyIn(), _abi.BodyPolyOut()
        i.step = float(step)
        hit, status, n_hit = np.full(K, -1, np.int64), np.zeros(K, np.uint8), np.zeros(1, np.int64)
        if K:
            o.hit, o.status = hit.ctypes.data, status.ctypes.data
        o.n_hit = n_hit.ctypes.data
        self._check(_abi.lib().mplx_body_check_poly(self._body, poly._h, C.byref(i), C.byref(o)))
        some = hit >= 0
        return {"hit": hit, "sample": np.where(some, hit >> 32, -1).astype(np.int32),
                "point": np.where(some, hit & 0xffffffff, -1).astype(np.int32), "status": status, "n_hit": int(n_hit[0])}

    def check_poly_resident(self, poly, step, hit=None, status=None, n_hit=None):
        """mplx_body_check_poly_device: asynchronous, on device buffers: hit [K] int64, status [K] bytes, n_hit 8 bytes
        that the call adds to; each may be None."""
        i, o = _abi.BodyPolyIn(), _abi.BodyPolyOut()
        i.step = float(step)
        for key, v in (("hit", hit), ("status", status), ("n_hit", n_hit)):
            if v is not None:
                setattr(o, key, _device_ptr(v))
        self._check(_abi.lib().mplx_body_check_poly_device(self._body, poly._h, C.byref(i), C.byref(o)))

    def free(self):
        b = self._body
        self._body = None
        if b and self._env._ctx:
            _abi.lib().mplx_body_destroy(b)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def load_traj_rows(env, rows, control=None):
    """One PolyTrajSet from host-side trajectories of different lengths (EnvMap.load_traj): rows = [(coeff [S_k][D + 1][6],
    dts [S_k])], as ShortcutResult.segments(k) returns them; trajectory k keeps its S_k segments."""
    S = max(len(d) for _, d in rows)
    c = np.zeros((S, env.dim + 1, 6, len(rows)))
    dts = np.ones((S, len(rows)))
    for k, (ck, dk) in enumerate(rows):
        c[:len(dk), :, :, k], dts[:len(dk), k] = ck, dk
    return env.load_traj(c, dts, n_segs=[len(d) for _, d in rows], control=control)


def refine_prioritised(env, plan, step, max_hop=None, control=None):
    """Shortcuts the robots of a plan_prioritised(keep=True) plan one after the other on the plan's clock, each against
    the CURRENT trajectories of all the others -- refined where already processed, raw otherwise -- held as one
    PolyTrajSet (load_traj_rows) in a reservation table filled PARK with the plan's t0 / radius / n_steps; the robot
    ignores its own group (mplx_shortcut_timed, include/mplx_reserve_poly.h).  A raw trajectory is the chain's own edges
    re-solved (a shortcut with max_hop = 1).  Robots are taken in the plan's order.  The pair test is symmetric and the
    instants are common, and a shortcut keeps a robot's ends and its total time, so the current set stays pairwise
    conflict-free at the instants as long as every chain_hit is -1.

    Returns {"trajs": the refined PolyTrajSet (free() it), "robots": the robot of each of its trajectories, "t0",
    "radius" [of those], "cost_before", "cost_after" [R] (the shortcut's chain_cost and cost; nan without a path),
    "chain_hit" [R] (-1: the chain holds), "refined" [R] bool, "conflicts": conflicts() over the refined set, PARK, rank =
    the position in the order}.

    Its limits: protection ends at the table's horizon (a hop that leaves it is not admitted; a chain that leaves it is
    reported with chain_hit -2); a robot with a chain hit keeps its raw chain and is reported, not replanned
    (replan_prioritised does that); the order is not revised, and a robot refined early is only ever refined against
    the RAW trajectories of the robots after it, so it cannot use room they give up later."""
    _no_body_plan("refine_prioritised", plan)
    R = len(plan["paths"])
    order, rad, t0, n_steps = plan["order"], np.asarray(plan["radius"], dtype=np.float64), plan["t0"], plan["n_steps"]
    chains = {r: plan["results"][r].full_path(plan["winner"][r]) for r in order if plan["paths"][r] is not None}
    before, after, hit = np.full(R, np.nan), np.full(R, np.nan), np.full(R, -1, np.int64)
    refined = np.zeros(R, dtype=bool)
    cur = {}
    for r, chain in chains.items():
        sc = _shortcut(env, [chain], 1, control)
        try:
            cur[r], before[r] = sc.segments(0), sc.cost[0]
        finally:
            sc.free()
    ctl = control
    for r, chain in chains.items():
        others = [k for k in cur if k != r]
        trajs = table = sc = None
        try:
            if others:
                trajs = load_traj_rows(env, [cur[k] for k in others], ctl)
                table = Reservations(env, trajs, step, n_steps, t0[others], rad[others], np.asarray(others, np.int32), True)
            else:
                table = Reservations(env, (np.zeros((env.n_fields, 0)), np.zeros((1, 0), np.int32)), step, n_steps, None, 0.0, None, True)
            sc = _shortcut(env, [chain], max_hop, control, table, [t0[r]], [rad[r]], [r])
            hit[r] = sc.chain_hit[0]
            after[r] = before[r]
            if hit[r] == -1 and sc.status[0] == 0:
                cur[r], after[r], refined[r] = sc.segments(0), sc.cost[0], True
        finally:
            for x in (sc, table, trajs):
                if x is not None:
                    x.free()
    robots = list(cur)
    out = {"robots": robots, "t0": t0[robots], "radius": rad[robots], "cost_before": before, "cost_after": after, "chain_hit": hit,
           "refined": refined, "trajs": None, "conflicts": None}
    if robots:
        rank = np.zeros(R, np.int32)
        rank[order] = np.arange(len(order), dtype=np.int32)
        out["trajs"] = load_traj_rows(env, [cur[k] for k in robots], ctl)
        out["conflicts"] = out["trajs"].conflicts(step, n_steps, t0=out["t0"], radius=out["radius"], rank=rank[robots], park=True)
    return out


def time_key(hashes, t):
    """mplx_time_key: the key of (lattice hash, t) in a table with time keys, element-wise."""
    h, tt = np.broadcast_arrays(np.asarray(hashes, dtype=np.uint64), np.asarray(t, dtype=np.float64))
    fn = _abi.lib().mplx_time_key
    return np.array([fn(int(a), float(b)) for a, b in zip(h.ravel(), tt.ravel())], dtype=np.uint64).reshape(h.shape)


def plan_prioritised(env, starts, goal_rows, step, radius, order=None, delays=(0.0,), park=True, wait=False, park_goal=False,
                     field=False, keep=False, best=None, **search_kw):
    """Prioritised planning of R robots on one map: robot r plans against the trajectories of the robots planned
    before it, as obstacles that move on the common clock of conflicts().  starts [4D+2][R] (t = 0 each), goal_rows
    [R][4D+2], radius a scalar or [R]; step: the clock's.  Robots are planned in `order` (default: the index, so a lower
    index has the higher priority).  Robot r is ONE search_many whose queries are its len(delays) start-delay
    candidates -- the same start and goal, t0[q] = delays[q], time keys on -- which share every launch; the winner is
    the found candidate with the smallest delays[q] + total time (ties: the smaller q).  Its chain joins the reservation
    table, which is refilled from the chosen chains with their t0.  search_kw goes to search_many; `n_steps` in it sets
    the table's horizon in instants (default: what covers max(delays) + 256 primitives); an edge past the horizon is
    blocked.

    Returns {"paths": [R] (start, actions) or None, "t0" [R], "status" [R] (of the winning candidate, else of
    candidate 0), "cost" [R] (g of the winner, inf), "conflicts": a final conflicts() over all chosen chains at `step`
    with rank = the position in `order`}.  keep=True: additionally "results" [R] -- each robot's MultiSearchResult, not
    freed and owned by the caller (free() them) --, "winner" [R] (the winning candidate, -1 without one), and "order",
    "n_steps" and "radius": what replan_prioritised continues with.  Without keep the function does what it always did.

    wait / park_goal go to search_many (EnvMap.search states them).  wait=True: standing still for one primitive is an
    edge (include/mplx_wait.h), so a robot can leave a lane, let another pass and go on, or stop short of a crossing;
    without it `delays` is the only way to wait, at the start only.  park_goal=True: a goal-region node counts as the
    goal only if the robot can stay there to the table's horizon without coming too close to a reservation
    (mplx_reserve_park_device); without it nothing is checked after a robot's own trajectory ends, and a later robot may
    park in the way of an earlier one, which only the final conflicts shows.  The two belong together: a robot whose
    early arrival is vetoed arrives later at the same lattice state through wait edges.

    field=True: the R goal distance fields (include/mplx_field.h) are built in one GoalField.build up front, and robot r
    searches with its own for every delay candidate.

    best=k goes to search_many (EnvMap.search states it): every delay candidate expands its k smallest keys a round.  It
    does nothing to optimality -- the stopping rule is unchanged -- and replan_prioritised keeps it.

    Its limits: a robot that finds no path is reported and not reserved.  Protection holds to the table's horizon
    (`n_steps`) only.  An earlier robot is never re-planned when a later one cannot avoid it (replan_prioritised replans every robot,
    in the same order, after the world has changed).  A chain with waits is not
    what rollout() / MapPlanner.checkTraj accept (they stop at a wait with SKIP_SAME), and smooth() / shortcut() of a
    path with repeated chain states only as shortcut(avoid=) and smooth(timed=True) take them (refine_prioritised; smooth(v=)
    re-allocates time and fails at a repeated state with SOLVE_BAD_TIME); traj_info / traj_sample / traj_traverse /
    conflicts take it as it is."""
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    goal_rows = np.ascontiguousarray(goal_rows, dtype=np.float64)
    if search_kw.get("body") is not None:
        raise ValueError("plan_prioritised: " + _BODY_REFUSED)
    if best is not None:
        search_kw = dict(search_kw, best=best)
    R = starts.shape[1]
    order = list(range(R)) if order is None else [int(r) for r in order]
    delays = np.atleast_1d(np.asarray(delays, dtype=np.float64))
    Q = delays.size
    rad = np.broadcast_to(np.asarray(radius, dtype=np.float64), (R,))
    dt = float(env._p.dt)
    n_steps = search_kw.pop("n_steps", None)
    if n_steps is None:
        n_steps = int(math.ceil((float(delays.max()) + 256 * dt) / float(step))) + 1
    paths, t0, status, cost = [None] * R, np.zeros(R), [None] * R, np.full(R, math.inf)
    results, winner = [None] * R, [-1] * R
    planned = []
    res = None
    fld = None
    try:
        if field:
            fld = GoalField(env).build(goal_rows, search_kw.get("tol_pos", 0.5))
            search_kw = dict(search_kw, field=fld)
        for r in order:
            if fld is not None:
                search_kw["field_of_query"] = [r] * Q
            st, ac = _path_set(env, [paths[k] for k in planned])
            fill = ((st, ac), step, n_steps, t0[planned], rad[planned] if planned else 0.0, None, park)
            if res is None:
                res = Reservations(env, *fill)
            else:
                res.fill(*fill)
            out = env.search_many(np.repeat(starts[:, r:r + 1], Q, axis=1), np.repeat(goal_rows[r:r + 1], Q, axis=0), avoid=res,
                                  t0=delays, radius=float(rad[r]), time_keys=True, wait=wait, park_goal=park_goal, **search_kw)
            try:
                best = None
                for q in range(Q):
                    if out.found[q]:
                        p = out.path(q)
                        end = float(delays[q]) + len(p[1]) * dt
                        if best is None or end < best[0]:
                            best = (end, q, p)
                status[r] = out.status[0 if best is None else best[1]]
                if best is not None:
                    paths[r], t0[r], cost[r] = best[2], float(delays[best[1]]), out.cost[best[1]]
                    planned.append(r)
                    winner[r] = best[1]
                if keep:
                    results[r], out = out, None
            finally:
                if out is not None:
                    out.free()
    except Exception:
        for o in results:
            if o is not None:
                o.free()
        raise
    finally:
        if res is not None:
            res.free()
        if fld is not None and not keep:  # (kept results go on searching with it: the caller frees it, plan["field"])
            fld.free()
    rank = np.zeros(R, np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    st, ac = _path_set(env, paths)
    final = env.traj_conflicts(st, ac, step, t0=t0, radius=rad, rank=rank, park=park)
    out = {"paths": paths, "t0": t0, "status": status, "cost": cost, "conflicts": final}
    if keep:
        out.update({"results": results, "winner": winner, "order": order, "n_steps": n_steps, "radius": rad.copy(), "field": fld})
    return out


def replan_prioritised(env, plan, now, step, radius=None, order=None, park=True, n_steps=None):
    """Replans a fleet that plan_prioritised(..., keep=True) planned, at time `now` of the common clock, after robots
    have moved, the map was edited or both: every robot, in the plan's order, runs replan_timed on its own table
    against the CURRENT plans of the robots before it.  Robot r finishes the primitive it is in: its root is chain state
    k_r = clip(ceil((now - t0_r) / dt), 0, len) of its full_path(); its t0 does not change.  The reservation table is
    refilled from the full_path()s of the robots already replanned, with their t0.  Of a robot's delay candidates only
    the winner is replanned; every loser gets a root that is out of range, which keeps nothing of it (it ends EMPTY).
    A robot without a path is reported (its old status) and skipped.  radius / order / n_steps default to the plan's.

    Returns the dict of plan_prioritised(keep=True) -- paths are full_path()s from the original starts, "results" the
    new MultiSearchResults (the plan's own entries are consumed: use the returned ones, and free() them) -- plus
    "rebase" [R]: the rebase result of each robot with "n_blocked", or None.

    plan["results"] is updated IN PLACE, entry by entry, as the robots are replanned (a replan consumes the result it
    is called on): if a later robot's replan raises, the plan still holds every live result -- the new ones of the
    robots already replanned, the old ones of the rest -- and the caller can free them or call again.

    Its limits: one table per robot stays allocated between calls.  The priority order is not revised: a robot is never
    asked to yield to one behind it.  A robot whose replan finds no path is not reserved, as in plan_prioritised, AND
    IS SKIPPED BY EVERY LATER CALL: its result has no path to advance along, so it stays where the failed replan left it
    until the caller plans it anew.  A plan made with field=True cannot be replanned after a map edit: its results
    search with the plan's GoalField (plan["field"], the caller's to free), which the edit makes stale, and replan_timed
    then raises RuntimeError as replan() does for a caller's stale field.  After a map edit such a fleet is planned anew."""
    _no_body_plan("replan_prioritised", plan)
    results, winner, t0 = plan["results"], list(plan["winner"]), np.array(plan["t0"], dtype=np.float64)
    R = len(results)
    order = list(plan["order"]) if order is None else [int(r) for r in order]
    rad = np.broadcast_to(np.asarray(plan["radius"] if radius is None else radius, dtype=np.float64), (R,))
    n_steps = int(plan["n_steps"] if n_steps is None else n_steps)
    dt = float(env._p.dt)
    paths, status, cost, rebase = [None] * R, list(plan["status"]), np.full(R, math.inf), [None] * R
    planned = []
    res = None
    try:
        for r in order:
            old, q = results[r], winner[r]
            if old is None or q < 0 or not old.found[q]:
                continue
            done = getattr(old, "_executed", None)
            n_done = 0 if done is None or done[q] is None else len(done[q][1])
            ids = old.table.path(old.goal_id[q])[0]
            k = int(min(max(math.ceil((float(now) - t0[r]) / dt), 0), n_done + len(ids) - 1))
            roots = [old.table.capacity] * old.n_queries  # (out of range: nothing of a loser is kept)
            roots[q] = int(ids[max(k - n_done, 0)])
            st, ac = _path_set(env, [paths[j] for j in planned])
            fill = ((st, ac), step, n_steps, t0[planned], rad[planned] if planned else 0.0, None, park)
            if res is None:
                res = Reservations(env, *fill)
            else:
                res.fill(*fill)
            new = old.replan_timed(avoid=res, roots=roots)
            results[r], rebase[r], status[r] = new, new.rebase_info, new.status[q]
            if new.found[q]:
                paths[r], cost[r] = new.full_path(q), new.cost[q]
                planned.append(r)
    finally:
        if res is not None:
            res.free()
    rank = np.zeros(R, np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    st, ac = _path_set(env, paths)
    final = env.traj_conflicts(st, ac, step, t0=t0, radius=rad, rank=rank, park=park)
    return {"paths": paths, "t0": t0, "status": status, "cost": cost, "conflicts": final, "results": results, "winner": winner,
            "order": order, "n_steps": n_steps, "radius": rad.copy(), "field": plan.get("field"), "rebase": rebase}


class _Result:
    """What SearchResult and MultiSearchResult share.  It owns the table, the open set and (search(field=True)) the goal
    field, and frees them; it holds the front end of replan / replan_timed and the paths of smooth / shortcut.  The
    two classes are views on it: MultiSearchResult shows per-query lists, SearchResult the values of its one query."""

    _multi, _who, _prior_word = True, "search_many", "priors"
    rebase_info = None  # of the rebase that made this result (a replan sets it)
    _executed = None  # per query (original start state, actions executed up to the root), set by replan_timed

    def __init__(self, status, last, table, open_set, rounds, expanded, total_rounds, env=None, params=None):
        self._env, self._params = env, params  # what replan() runs again with
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
        self.field, self._owns_field, self._field_of_query = None, False, None  # (search(field=): _hand_field)

    @classmethod
    def _of(cls, status, last, table, open_set, rounds, expanded, total_rounds, env, params):
        """The result of a run that counted per query."""
        return cls(status, last, table, open_set, rounds, expanded, total_rounds, env, params)

    def _per_query(self, name):
        v = getattr(self, name)
        return v if self._multi else [v]

    def _chain(self, goal_id):
        ids, act = self.table.path(goal_id)
        return self.table.state_of(ids[0]), act

    def _full_path(self, q):
        start, act = self._path_of(q)
        done = None if self._executed is None else self._executed[q]
        if done is None:
            return start, act
        return done[0].copy(), np.concatenate([done[1], act]).astype(np.int32)

    def smooth(self, v=1.0, control=None, timed=False, avoid=None):
        """The path(s) smoothed into polynomials through their chain states (include/mplx_solve.h): v a scalar or [n_v]
        speeds of the time allocation -> a PolyTrajSet of Q x n_v problems in one solve, problem vi * Q + q = the path of
        query q at speed v[vi] (Q = 1 for a SearchResult); control: of the ends (default: the EnvMap's).  Of a
        MultiSearchResult a query without a path is SOLVE_EMPTY.

        timed=True: the chain's own times instead of a time allocation (v must be left at its default): Q problems, the
        chain full_path(q), segment s lasts t_{s+1} - t_s of the chain states, so the robot stays on the clock it was
        planned on and the repeated states of wait edges are legal.  The set's chain_times [w_max][Q] are those t.  avoid
        (with timed): a Reservations; the result is checked against it with the t0 / radius / ignore_group the search
        ran with (Reservations.check_poly) and the dict is the set's reserve_hit -- a smoothed trajectory is NOT kept
        clear of the reservations, only reported.

        Of a search that ran with a body (EnvMap.search(body=)) this returns what it returns without one: the output is
        NOT body-checked.  Body.check_poly(the returned set, step) reports where the smoothed body touches the cloud."""
        if not timed:
            if avoid is not None:
                raise ValueError("smooth: avoid goes with timed=True")
            return _smooth(self._env, self._paths(), v, control)
        if np.ndim(v) != 0 or float(v) != 1.0:
            raise ValueError("smooth: timed=True keeps the chain's own times: leave v at its default")
        prm = self._params or {}
        if avoid is not None and not prm.get("avoid"):
            raise ValueError("smooth: the search ran without avoid (no t0 / radius to check with)")
        return _smooth_timed(self._env, self._full_paths(), control, avoid, prm.get("t0"), prm.get("radius"), prm.get("ignore_group"))

    def _full_paths(self):
        return [self._full_path(q) if self.found[q] else None for q in range(self.n_queries)]

    def shortcut(self, max_hop=None, control=None, avoid=None):
        """The path(s) with runs of their short constant-control pieces replaced by two-point primitives between
        non-adjacent chain states, where those stay within v_max / a_max / j_max and off the obstacles and cost less
        (mplx_shortcut, include/mplx_limits.h): a ShortcutResult of Q queries in one batch of launches.  max_hop: the
        longest hop in chain states (default: any).  Of a MultiSearchResult a query without a path is SOLVE_EMPTY.

        avoid: a Reservations as they are now: the timed shortcut (mplx_shortcut_timed, include/mplx_reserve_poly.h) with
        the t0 / radius / ignore_group the search ran with, on the chain full_path(q), whose clock is the original
        start's: a hop is admitted only if it stays clear of the reservations inside the table's horizon, and
        ShortcutResult.chain_hit reports a chain that no longer holds (replan_timed then).  A search that ran with avoid
        must be shortcut with it: an untimed hop across its waits would drift into what the search waited for.

        Of a search that ran with a body (EnvMap.search(body=)) this returns what it returns without one: a hop is tested
        as a point against the map and the output is NOT body-checked.  Body.check_poly(result.poly, step) reports where
        the shortcut body touches the cloud."""
        prm = self._params or {}
        if prm.get("avoid") and avoid is None:
            raise ValueError("shortcut: the search ran with avoid: give the Reservations as they are now")
        if avoid is None:
            return _shortcut(self._env, self._paths(), max_hop, control)
        if not prm.get("avoid"):
            raise ValueError("shortcut: the search ran without avoid (no t0 / radius to check with)")
        return _shortcut(self._env, self._full_paths(), max_hop, control, avoid, prm["t0"], prm["radius"], prm["ignore_group"])

    def _roots(self, who, roots, advance):
        """The node id every query is re-rooted at: roots [Q] (-1 or None: that query's seed), or ids[advance] of the
        chain its path follows."""
        Q = self.n_queries
        r = [-1] * Q
        if roots is not None:
            r = [-1 if x is None else int(x) for x in np.broadcast_to(np.asarray(roots, dtype=object), (Q,))]
        if advance is not None:
            found, goal_id = self._per_query("found"), self._per_query("goal_id")
            if not self._multi and not found[0]:
                raise RuntimeError("%s: advance needs a path (status %s)" % (who, STATUS_NAMES[self.status]))
            ks = np.broadcast_to(np.asarray(advance, dtype=np.int64), (Q,))
            r = [int(self.table.path(goal_id[q])[0][int(ks[q])]) if found[q] else -1 for q in range(Q)]
        return r

    def _replan(self, who, roots, advance, goal_rows, check_edges, priors, timed=False, avoid=None):
        if self.table is None or self._params is None:
            raise RuntimeError("%s: this result does not own a table (it was replanned or freed)" % who)
        _no_body(who, self._params)
        if timed:
            _need_timed(self._params, avoid)
        else:
            _no_replan(self._params)
        if roots is not None and advance is not None:
            raise ValueError("%s: give %s or advance, not both" % (who, "roots" if self._multi else "root"))
        return run_replan(self, self._multi, self._roots(who, roots, advance), goal_rows, check_edges, priors, timed, avoid)

    rekey_info = None  # per query, of the re-key that made this result (improve sets it)
    _pruned_at = None  # per query the smallest cut an improve pruned its open nodes with (None: never)

    def _certificate(self):
        """Per query (slack, certified): slack = w * tol_pos / v_max (w * tol_pos for v_max <= 0) -- h is measured to the
        goal's centre while the goal test accepts a box, so h - slack is what is admissible --; certified: the heuristic
        the open set pushes with is, less slack, a lower bound of the cost to go: the default, a goal field, and "robust"
        with every tolerance zero; not priors, not "robust" on a goal box."""
        Q, kw, p = self.n_queries, self._params["goal_kw"], self._env._p
        per = lambda v, default=None: np.broadcast_to(np.asarray(default if v is None else v, dtype=np.float64), (Q,))
        w, v_max, tol = per(kw["w"], p.w), per(kw["v_max"], p.v_max), per(kw["tol_pos"])
        slack = [float(w[q] * tol[q] / v_max[q]) if v_max[q] > 0 else float(w[q] * tol[q]) for q in range(Q)]
        exact = [all(per(kw[k])[q] == 0 for k in ("tol_pos", "tol_vel", "tol_acc", "tol_yaw")) for q in range(Q)]
        opn = self.open
        cert = [(not opn.has_priors) and (opn.heur_mode is None or exact[q]) for q in range(Q)]
        return slack, cert

    def _bound(self):
        if self.table is None or self._params is None:
            raise RuntimeError("bound: this result does not own a table (it was replanned, improved or freed)")
        slack, cert = self._certificate()
        rk = self.open.rekey(self._params["eps"], write=False)
        g_max, cost = float(self._params["g_max"]), self._per_query("cost")
        cuts = self._pruned_at or [math.inf] * self.n_queries
        out = []
        for q in range(self.n_queries):
            # what cut the tree bounds nothing above itself: g_max, and the cut of a pruning improve (a pruned node had
            # g + h >= cut, and is no longer open to say so)
            lower = max(0.0, min(rk[q]["lower"], g_max, cuts[q]) - slack[q])
            ratio = math.nan
            if cert[q]:
                ratio = cost[q] / lower if lower > 0 else (1.0 if cost[q] == 0 else math.inf)
            out.append({"cost": cost[q], "lower": lower, "slack": slack[q], "ratio": ratio, "certified": cert[q],
                        "n_open": rk[q]["n_open"]})
        return out

    def _improve(self, eps, prune, max_rounds, max_expand, avoid):
        if self.table is None or self._params is None:
            raise RuntimeError("improve: this result does not own a table (it was replanned, improved or freed)")
        prm = self._params
        if prm.get("avoid") and avoid is None:
            raise ValueError("improve: the search ran with avoid: give the Reservations as they are now")
        if avoid is not None and not prm.get("avoid"):
            raise ValueError("improve: the search ran without avoid (no t0 / radius to check with)")
        eps = float(eps)
        if not (eps >= 0.0) or math.isinf(eps):
            raise ValueError("improve: eps must be finite and >= 0")
        return run_improve(self, self._multi, eps, prune, max_rounds, max_expand, avoid)

    def _hand_field(self, old=None, field=None, owned=False, foq=None):
        """The field of this result: from the search that made it, or handed on by the result `old` a replan consumed."""
        if old is not None:
            field, owned, foq = old.field, old._owns_field, old._field_of_query
            old.field, old._owns_field = None, False
        self.field, self._owns_field, self._field_of_query = field, owned, foq

    def free(self):
        if self.open is not None:
            self.open.free()
        if self.table is not None:
            self.table.free()
        self.open = self.table = None
        if self._owns_field and self.field is not None:
            self.field.free()
        self.field, self._owns_field = None, False


def _one_goal(goal_row):
    return None if goal_row is None else np.array(goal_row, dtype=np.float64).reshape(1, -1)


class SearchResult(_Result):
    """What EnvMap.search returns.  status: FOUND, EMPTY (no open node left: the goal region is not reachable within
    g_max), MAX_ROUNDS or MAX_EXPAND (stopped early; the nodes selected last are open again); cost: g of the goal node
    (inf unless FOUND); rounds = relax calls made; expanded = nodes expanded (a re-opened node counts again); table and
    open: the NodeTable and OpenSet, owned by the result -- free() it (or let it go) before the EnvMap is closed."""

    _multi, _who, _prior_word = False, "search", "prior"

    def __init__(self, status, last, table, open_set, rounds, expanded, env=None, params=None):
        super().__init__([status], [last], table, open_set, [rounds], [expanded], rounds, env, params)
        self.status, self.found, self.goal_id, self.cost = self.status[0], self.found[0], self.goal_id[0], self.cost[0]
        self.last_select, self.rounds, self.expanded = last, rounds, expanded

    @classmethod
    def _of(cls, status, last, table, open_set, rounds, expanded, total_rounds, env, params):
        return cls(status[0], last[0], table, open_set, total_rounds, expanded[0], env, params)

    def path(self):
        """(start_state, actions) of the chain of best predecessors from the seed to the goal node: the `starts` and
        `actions` (reshape(-1, 1)) of EnvMap.rollout / traj_*."""
        if not self.found:
            raise RuntimeError("search: no path (status %s)" % STATUS_NAMES[self.status])
        return self._chain(self.goal_id)

    def _path_of(self, q):
        return self.path()

    def _paths(self):
        return [self.path()]

    def as_prior(self):
        """This result's path as the Prior of a later search (with the control set this search ran with)."""
        return _prior_of(self, None)

    def replan(self, root=None, advance=None, goal_row=None, check_edges=True, prior=None):
        """Plans again on the table of this search after the robot has moved and / or the map was edited
        (include/mplx_replan.h), with the parameters of the search that made this result.  root: the
        node id the robot is at (default: the seed); advance=k: ids[k] of the chain path() follows.  Nodes that still
        hang below the root by edges valid on the map as it is now keep their g -- costs go on being measured from the
        original start --, all of them are expanded once in a forced round (in chunks of max_frontier rows), then the
        loop of EnvMap.search finishes.  goal_row: a new goal; keys and goal bits of the kept nodes are recomputed
        anyway.  A search with a prior replans with it (the open set keeps it); a new goal_row drops it unless `prior`
        gives one again.  A search with a field replans with it: a field the search built itself (field=True) is rebuilt in
        place when it is stale or a new goal_row is given; a caller's field that is stale, or a new goal_row with a
        caller's field, raises -- rebuild the field and search anew.  Returns a new SearchResult that owns the table and
        the open set; this one no longer does."""
        return self._replan("replan", root, advance, _one_goal(goal_row), check_edges, None if prior is None else [prior])

    def replan_timed(self, avoid=None, root=None, advance=None, goal_row=None, check_edges=True):
        """replan() for a search that ran with time keys and / or among reservations (include/mplx_replan_timed.h;
        DESIGN.md 4.22).  The robot's clock does not move: g and t go on being measured from the original start and the
        t0 the search ran with stays, so t0 + t is still the common clock of conflicts() and the time keys of the kept
        nodes are still right.  avoid: the Reservations as they are NOW (the same object refilled, or another one);
        required iff the search ran with avoid.  Its queries are set again from the t0, radius and ignore_group of the
        search.  A kept edge must still hold on the map (check_edges), a wait edge by the wait's own rule, and must
        keep clear of the reservations; the kept nodes are pushed closed, vetoed where the robot could not stay
        (park_goal) and expanded once in a forced round with the waits, the check and the veto of the search.  A
        search without time keys and without avoid is refused with ValueError: replan() is for it.  root / advance /
        goal_row and the handling of priors and fields: as replan().  Returns a new SearchResult that owns the table
        and the open set; its path() starts at the root, whose t is not 0 -- full_path() is the chain from the original
        start."""
        return self._replan("replan_timed", root, advance, _one_goal(goal_row), check_edges, None, True, avoid)

    def bound(self):
        """How far the cost in hand can be from the optimum (include/mplx_anytime.h), from one pass over
        the table that changes nothing: {"cost", "lower", "slack", "ratio", "certified", "n_open"}.  lower =
        max(0, min(L_min, g_max, cut) - slack) with L_min the smallest g + h among the open nodes and cut what an
        improve(prune=True) closed open nodes at (inf: never): after any completed round
        some open node on an optimal path carries its optimal g, so no path that is cheaper than `cost` costs less than
        `lower` -- the optimum is at least min(cost, lower).  ratio = cost / lower: cost <= ratio * optimum; a ratio
        <= 1 proves the cost optimal (up to slack).  certified False (priors, "robust" on a goal box): h is no lower
        bound, lower is still reported and ratio is nan.  Not valid on a table with a status bit (the call raises), nor
        after a replan that was interrupted before its forced chunks finished."""
        return self._bound()[0]

    def improve(self, eps, prune=True, max_rounds=None, max_expand=None, avoid=None):
        """Searches on with another eps on the tree this search has paid for (include/mplx_anytime.h):
        every key of the table is recomputed as g + eps * h (OpenSet.rekey), then the loop of EnvMap.search finishes.
        Nothing is re-rooted and no node is expanded for its own sake: a closed node is expanded again only if its g
        falls (the push re-opens it).  prune: of a query that is FOUND and certified (bound()) the open nodes with
        g + h >= cost + slack are closed by the re-key -- none of them can lead below the cost in hand; False closes
        nothing.  max_rounds / max_expand: limits of this call alone (None: none); rounds and expanded of the new
        result count on from this one's.  The field, priors, heuristic mode, best, wait / park_goal and time keys of the
        search stay; a stale field is an error of the re-key (replan rebuilds one).  avoid: the Reservations as they are
        now, required iff the search ran with avoid.  A later replan / replan_timed uses the new eps.  Returns a new
        result that owns the table and the open set; this one no longer does."""
        return self._improve(eps, prune, max_rounds, max_expand, avoid)

    def full_path(self):
        """(start_state, actions) from the ORIGINAL start (t = 0): the actions executed up to the root of every
        replan_timed so far, then those of path().  This is the chain conflicts() and a reservation fill take with the
        robot's unchanged t0; for a result that was never replanned it is path().  The positions the check computed
        along it and those of traj_sample agree bit for bit: both evaluate the segment of (chain state, control) at the
        local time tl_i - t of that state."""
        return self._full_path(0)

    def __repr__(self):
        return "SearchResult(%s, cost=%r, rounds=%d, expanded=%d)" % (STATUS_NAMES[self.status], self.cost, self.rounds, self.expanded)


class MultiSearchResult(_Result):
    """What EnvMap.search_many returns: per query q status[q] (FOUND, EMPTY, MAX_ROUNDS or MAX_EXPAND), found[q], cost[q]
    (inf unless FOUND), goal_id[q] (a global node id, -1 unless FOUND), rounds[q] (the rounds in which q selected) and
    expanded[q]; total_rounds = relax calls made.  last_select: the Q results of the last select.  table and open are
    owned by the result: free() it (or let it go) before the EnvMap is closed."""

    def path(self, q):
        """(start_state, actions) of query q, as SearchResult.path."""
        if not self.found[q]:
            raise RuntimeError("search_many: no path for query %d (status %s)" % (q, STATUS_NAMES[self.status[q]]))
        return self._chain(self.goal_id[q])

    _path_of = path

    def _paths(self):
        return [self.path(q) if self.found[q] else None for q in range(self.n_queries)]

    def as_priors(self):
        """[Q] Prior (None for a query without a path): the `priors` of a later search_many."""
        return [_prior_of(self, q) if self.found[q] else None for q in range(self.n_queries)]

    def conflicts(self, step, n_steps=None, t0=None, radius=None, group=None, rank=None, park=True, want_pairs=False, chunk_steps=0):
        """Conflicts between the Q raw paths on a common clock (EnvMap.traj_conflicts on the chains of path(q), with the
        parameters and controls the EnvMap holds now): a ConflictResult of Q entries; a query without a path is excluded
        (TRAJ_EMPTY)."""
        starts, actions = _path_set(self._env, self._paths())
        return self._env.traj_conflicts(starts, actions, step, n_steps=n_steps, t0=t0, radius=radius, group=group, rank=rank,
                                        park=park, want_pairs=want_pairs, chunk_steps=chunk_steps)

    def replan(self, roots=None, advance=None, goal_rows=None, check_edges=True, priors=None):
        """SearchResult.replan for Q queries at once: roots [Q] (node ids; -1 or None: that query's seed), or advance
        (one k for all or [Q]; a query without a path keeps its seed), goal_rows [Q][4D+2] or None.  Every launch of
        the rebase, of the forced round and of the rounds after it is shared by the queries.  Returns a new
        MultiSearchResult that owns the table and the open set; this one no longer does."""
        return self._replan("replan", roots, advance, goal_rows, check_edges, priors)

    def replan_timed(self, avoid=None, roots=None, advance=None, goal_rows=None, check_edges=True):
        """SearchResult.replan_timed for Q queries at once: roots [Q] (node ids; -1 or None: that query's seed; an id
        that is out of range keeps nothing of the query, which then ends EMPTY), or advance (one k for all or [Q]; a
        query without a path keeps its seed), goal_rows [Q][4D+2] or None.  Returns a new MultiSearchResult that owns
        the table and the open set; this one no longer does."""
        return self._replan("replan_timed", roots, advance, goal_rows, check_edges, None, True, avoid)

    def bound(self):
        """SearchResult.bound per query: a list of Q dicts."""
        return self._bound()

    def improve(self, eps, prune=True, max_rounds=None, max_expand=None, avoid=None):
        """SearchResult.improve for Q queries at once: one re-key and the shared rounds of search_many; a query is pruned
        by its own cost.  Returns a new MultiSearchResult that owns the table and the open set; this one no longer
        does."""
        return self._improve(eps, prune, max_rounds, max_expand, avoid)

    def full_path(self, q):
        """SearchResult.full_path of query q."""
        return self._full_path(q)

    def __repr__(self):
        return "MultiSearchResult(%s, rounds=%d, expanded=%d)" % (
            [STATUS_NAMES[st] for st in self.status], self.total_rounds, sum(self.expanded))


def _need_timed(prm, avoid):
    if not (prm.get("avoid") or prm.get("time_keys")):
        raise ValueError("replan_timed: the search ran without time keys and without avoid: use replan")
    if prm.get("avoid") and avoid is None:
        raise ValueError("replan_timed: the search ran with avoid: give the Reservations as they are now")
    if avoid is not None and not prm.get("avoid"):
        raise ValueError("replan_timed: the search ran without avoid (no t0 / radius to check with)")


def _no_replan(prm):
    if prm.get("avoid") or prm.get("time_keys"):
        raise RuntimeError("replan: the search ran among reservations or with time keys: use replan_timed "
                           "(include/mplx_replan_timed.h)")


_BODY_REFUSED = ("a search with a body (include/mplx_body.h) cannot be replanned or planned in priority order: the rebase "
                 "does not re-test bodies; search anew")


def _no_body(who, prm):
    if prm is not None and prm.get("body") is not None:
        raise RuntimeError("%s: %s" % (who, _BODY_REFUSED))


def _no_body_plan(who, plan):
    for r in plan.get("results") or []:
        _no_body(who, getattr(r, "_params", None))


def _body_setup(who, body, body_samples, prm):
    """The `body` / `body_samples` arguments of a search: the Body every round's lists are checked against, the samples per
    edge, the generation of its cloud (improve and anytime refuse another one)."""
    if not isinstance(body, Body):
        raise TypeError("%s: body must be a search.Body (EnvMap.alloc_body)" % who)
    if int(body_samples) < 1:
        raise ValueError("%s: body_samples must be >= 1" % who)
    sh = body.shape()
    if not sh["cells"].any():
        raise ValueError("%s: the body has no cloud: fill() it first (an empty cloud is fine)" % who)
    prm["body"], prm["body_samples"], prm["body_generation"] = body, int(body_samples), sh["generation"]


def _body_current(who, prm):
    body = prm.get("body")
    if body is not None and body.generation != prm["body_generation"]:
        raise RuntimeError("%s: the body's cloud was filled again since the search (generation %d, the search ran with %d): "
                           "the tree was built against another cloud; search anew" % (who, body.generation, prm["body_generation"]))


def _avoid_setup(who, avoid, time_keys, starts, Q, t0, radius, ignore_group, tab, prm, wait=False, park_goal=False):
    """The `avoid` / `time_keys` / `wait` / `park_goal` arguments of a search: checks, the queries of the reservation
    table, the table's keys."""
    time_keys = (avoid is not None) if time_keys is None else bool(time_keys)
    if wait and not time_keys:
        raise ValueError("%s: wait needs time keys (the key of a wait would be its parent's)" % who)
    if park_goal and avoid is None:
        raise ValueError("%s: park_goal needs avoid (the reservation table a goal node is held against)" % who)
    prm["avoid"], prm["time_keys"] = avoid is not None, time_keys
    prm["wait"], prm["park_goal"] = bool(wait), bool(park_goal)
    if avoid is not None:
        if radius is None:
            raise ValueError("%s: avoid needs a radius" % who)
        if np.any(np.asarray(starts)[-1] != 0.0):
            raise ValueError("%s: with avoid a start state must have t = 0 (the robot's clock is t0 + t)" % who)
        # (kept for replan_timed, which sets the queries of its reservation table again)
        prm["t0"] = np.array(np.broadcast_to(np.asarray(t0, dtype=np.float64), (Q,)))
        prm["radius"] = np.array(np.broadcast_to(np.asarray(radius, dtype=np.float64), (Q,)))
        prm["ignore_group"] = np.array(np.broadcast_to(np.asarray(ignore_group, dtype=np.int32), (Q,)))
        avoid.set_queries(prm["t0"], prm["radius"], prm["ignore_group"])
    if time_keys:
        tab.set_time_keys(True)


def _table_check(tab, who, where):
    status = tab.stats()[1]  # (the stream is idle: no copy, no wait)
    if status:
        raise RuntimeError("%s: table status %d %s (1 nodes full, 2 probe full, 4 frontier full): raise capacity"
                           % (who, status, where))


def _edges(prm, avoid):
    """(wait, park) of a round: wait edges join the lists before the check (include/mplx_wait.h); every push is followed
    by the park veto of `avoid` (mplx_reserve_park_device)."""
    return bool(prm.get("wait")), bool(prm.get("park_goal")) and avoid is not None


def _round(env, tab, opn, avoid, rows, imp, lists, n, prm, wait, park):
    """One round on the n rows of `rows` (a selection, or a chunk of the nodes a rebase kept): expand them, append the
    wait edges, check the lists against the reservations of `avoid` (the edges it blocks cost +inf, which the relax
    skips), check them against the cloud of prm["body"] (include/mplx_body.h: the same +inf), relax the lists against the
    table, push the nodes whose g fell, veto the goal nodes the robot could not stay at.  With avoid None, wait and park
    off and no body these are the calls of a search without them."""
    env.expand_lists_resident(rows, lists, n_nodes=n)
    if wait:
        _add_waits(env, avoid, rows, lists, n)
    if avoid is not None:
        avoid.check(rows, lists, n, table=tab)
    if prm.get("body") is not None:
        prm["body"].check(rows, lists, n, prm["body_samples"])
    tab.relax(lists, rows.id, rows.g, prm["g_max"], frontier=imp, n_nodes=n, want_count=False)
    opn.push(imp, n_max=n * lists.stride, eps=prm["eps"], sight=prm["sight"])
    if park:
        avoid.park(opn, imp, n * lists.stride)


def _search_loop(env, who, multi, tab, opn, sel, imp, lists, prm, total, rounds, expanded, avoid=None):
    """The rounds of a search from its first select on: select (the round's only read-back), and while any query
    selects: one _round on the selection.  rounds / expanded: per query (one entry for a table of one query), counted
    on from what they hold.  avoid: a Reservations whose check runs between the expansion and the relax; None: the calls
    of a search without one.  prm["wait"] / prm["park_goal"]: _edges.  With both off the loop issues exactly the calls it
    issued before they existed.  prm["best"]: the selects are those of include/mplx_best.h; None: the plain ones.  Returns (status per query, the results of the last select, relax calls made)."""
    eps, delta, sight = prm["eps"], prm["delta"], prm["sight"]
    wait, park = _edges(prm, avoid)
    max_rounds, max_expand = prm["max_rounds"], prm["max_expand"]
    best = prm.get("best")
    limit = None
    while True:
        try:
            if best is None:
                res = opn.select_many(delta, sel) if multi else [opn.select(delta, sel)]
            else:
                res = opn.select_many(delta, sel, best=best) if multi else [opn.select(delta, sel, best=best)]
        except _abi.MplxError as e:
            if e.code != _abi.ERR_STATE:
                raise
            _table_check(tab, who, "in round %d" % total)
            raise
        n = sum(r["count"] for r in res)
        if not any(r["status"] == SELECTED for r in res):
            break
        limit = MAX_ROUNDS if (max_rounds is not None and total >= max_rounds) else \
            MAX_EXPAND if (max_expand is not None and sum(expanded) + n > max_expand) else None
        if limit is not None:
            opn.push(sel, n_max=n, eps=eps, sight=sight)  # the selection is open again: same g, same keys
            if park:
                avoid.park(opn, sel, n)
            break
        _round(env, tab, opn, avoid, sel, imp, lists, n, prm, wait, park)
        total += 1
        for q, r in enumerate(res):
            if r["status"] == SELECTED:
                rounds[q] += 1
                expanded[q] += r["count"]
    status = [limit if (r["status"] == SELECTED and limit is not None) else r["status"] for r in res]
    return status, res, total


def _add_waits(env, avoid, sel, lists, n):
    """The wait edges of a round: Reservations.add_waits, or the same call without a reservation table (a search with
    time keys and wait but no avoid)."""
    if avoid is not None:
        avoid.add_waits(sel, lists, n)
        return
    s = lists.c_struct()
    _abi.check(env._ctx, _abi.lib().mplx_lists_add_wait_device(env._ctx, C.byref(s), int(n), int(sel.ptr), int(sel.n_nodes),
                                                               _device_ptr(sel.id), None))


def _params(env, eps, delta, g_max, max_rounds, max_expand, capacity, max_frontier, lists_stride, sight, goal_kw, best=None, Q=1):
    if delta is None:
        delta = float(env._p.w) * float(env._p.dt)
    if best is not None:
        best = int(best)
        if best < 1:
            raise ValueError("best must be >= 1")
    # with best no select takes more than best rows per query: the frontier and the lists need no more
    fcap = int(max_frontier) if max_frontier is not None else int(capacity) if best is None else min(int(capacity), best * int(Q))
    return {"eps": eps, "delta": delta, "g_max": g_max, "max_rounds": max_rounds, "max_expand": max_expand,
            "capacity": int(capacity), "fcap": fcap, "best": best,
            "lists_stride": lists_stride, "sight": sight, "goal_kw": goal_kw,
            # what as_prior() hands on: the control set of this search
            "control": int(env._p.control), "U": getattr(env, "_U_host", None), "dt": float(env._p.dt)}


def _own(stack, obj):
    """`obj` is freed when the ExitStack `stack` unwinds (unless its pop_all() was called first)."""
    stack.callback(obj.free)
    return obj


class _Scratch(list):
    """The frontiers and lists of one run, freed together in the order they were made."""

    def add(self, buf):
        self.append(buf)
        return buf

    def free(self):
        for b in self:
            b.free()


def run_search(env, start, goal_row, prior=None, **opts):
    """EnvMap.search: the query as [4D+2][1] / [1][4D+2]."""
    return _run(env, False, np.asarray(start, dtype=np.float64).reshape(-1, 1), _one_goal(goal_row),
                dict(opts, priors=None if prior is None else [prior]))


def run_search_many(env, starts, goal_rows, **opts):
    starts = np.ascontiguousarray(starts, dtype=np.float64)
    goal_rows = np.ascontiguousarray(goal_rows, dtype=np.float64)
    if starts.ndim != 2 or goal_rows.ndim != 2 or starts.shape[0] != env.n_fields or goal_rows.shape != (starts.shape[1], env.n_fields):
        raise ValueError("search_many: starts must be [%d][Q] and goal_rows [Q][%d]" % (env.n_fields, env.n_fields))
    if starts.shape[1] < 1:
        raise ValueError("search_many: no query")
    return _run(env, True, starts, goal_rows.copy(), opts)


def _run(env, multi, starts, goal_rows, opts):
    """EnvMap.search (multi=False) and EnvMap.search_many: starts [4D+2][Q], goal_rows [Q][4D+2], opts: the keyword
    arguments of EnvMap.search_many.  The two differ in the calls named at the branches on `multi` (here, in
    _search_loop and in run_replan) and in nothing else: a search of one query keeps its goal on the context, has no
    query column and selects with mplx_open_select_device."""
    cls = MultiSearchResult if multi else SearchResult
    who, prior_word = cls._who, cls._prior_word
    priors, field, heur, avoid, park_goal = opts["priors"], opts["field"], opts["heur"], opts["avoid"], opts["park_goal"]
    if field is not None and field is not False and priors is not None:
        raise ValueError("%s: field and %s exclude each other" % (who, prior_word))
    if heur is not None and priors is not None:
        raise ValueError("%s: heur and %s exclude each other" % (who, prior_word))
    env._flush()
    Q = starts.shape[1]
    prm = _params(env, *(opts[k] for k in ("eps", "delta", "g_max", "max_rounds", "max_expand", "capacity", "max_frontier",
                                           "lists_stride", "sight")),
                  {k: opts[k] for k in ("w", "v_max", "tol_pos", "tol_vel", "tol_acc", "tol_yaw")}, opts.get("best"), Q)
    prm["goal_rows"] = goal_rows
    # the open set carries its goals itself (several queries and priors need that): replan keeps it so
    prm["own_goals"] = multi or priors is not None
    eps, sight, fcap, capacity = prm["eps"], prm["sight"], prm["fcap"], prm["capacity"]
    g0 = None if opts["start_g"] is None else np.broadcast_to(np.asarray(opts["start_g"], dtype=np.float64), (Q,))
    if g0 is not None and not g0.any():
        g0 = None  # (the call without a g row: the bytes of a search before start_g existed)
    if not multi:
        env.set_goal(goal_rows[0], **prm["goal_kw"])
    with contextlib.ExitStack() as always, contextlib.ExitStack() as owned:  # (owned: freed on failure only)
        scratch = _own(always, _Scratch())
        tab = _own(owned, NodeTable(env, capacity, n_queries=Q))
        if avoid is not None or opts["time_keys"] or opts["wait"] or park_goal:
            _avoid_setup(who, avoid, opts["time_keys"], starts, Q, opts["t0"], opts["radius"], opts["ignore_group"], tab, prm,
                         opts["wait"], park_goal)
        if opts.get("body") is not None:
            _body_setup(who, opts["body"], opts.get("body_samples", 4), prm)
        opn = _own(owned, OpenSet(env, tab))
        if prm["own_goals"]:
            opn.set_goals(goal_rows, **prm["goal_kw"])
        if priors is not None:
            opn.set_prior_list(list(priors))
        fld, fld_owned, foq = _field_setup(who, env, opn, field, opts["field_of_query"], goal_rows, opts["tol_pos"], priors)
        if fld_owned:
            owned.callback(fld.free)
        if heur is not None:  # (the open set keeps the mode: a replan pushes with it)
            opn.set_heur(heur)
        # (imp: no more nodes can improve than exist)
        sel, imp = scratch.add(TableFrontier(env, fcap)), scratch.add(TableFrontier(env, capacity))
        lists = scratch.add(env.alloc_lists(fcap, want_state=True, stride=prm["lists_stride"]))
        count = tab.seed(starts, g0, frontier=imp, query=np.arange(Q, dtype=np.int32) if multi else None)
        _table_check(tab, who, "after seeding")
        opn.push(imp, n_max=count, eps=eps, sight=sight)
        if park_goal:
            avoid.park(opn, imp, count)
        rounds, expanded = [0] * Q, [0] * Q
        status, res, total = _search_loop(env, who, multi, tab, opn, sel, imp, lists, prm, 0, rounds, expanded, avoid)
        out = cls._of(status, res, tab, opn, rounds, expanded, total, env, prm)
        out._hand_field(None, fld, fld_owned, foq)
        owned.pop_all()  # the result owns them now
        return out


def _executed(old, tab, roots):
    """Per query (original start state, actions executed so far), or None: what `old` holds, extended by the chain from
    the table's current root to the new one -- taken before the rebase cuts it."""
    Q = len(roots)
    before = old._executed or [None] * Q
    n = tab.stats()[0]
    out = []
    for q, r in enumerate(roots):
        done = before[q]
        if 0 <= r < n:
            ids, act = tab.path(r)
            if done is None:
                done = (tab.state_of(ids[0]), np.zeros(0, np.int32))
            done = (done[0], np.concatenate([done[1], act]).astype(np.int32))
        out.append(done)
    return out


def run_replan(old, multi, roots, goal_rows, check_edges, priors=None, timed=False, avoid=None):
    """SearchResult.replan / MultiSearchResult.replan: rebase into a frontier of the table's capacity, clear the open
    set, push the kept nodes closed, expand all of them in chunks of max_frontier rows (the forced round: one _round per
    chunk), then the loop of the search.  The forced chunks count as rounds and expansions.  timed: replan_timed -- the
    rebase is rebase_timed against `avoid`, and the forced round runs the waits, the check and the park veto of the
    search's rounds; without it the calls are those of replan.  roots [Q] node ids, goal_rows [Q][4D+2] or None."""
    env, prm, tab, opn = old._env, old._params, old.table, old.open
    who = "replan_timed" if timed else "replan"
    if not timed:
        avoid = None
    wait, park = _edges(prm, avoid)
    if avoid is not None:
        avoid.set_queries(prm["t0"], prm["radius"], prm["ignore_group"])
    env._flush()
    eps, sight, fcap, capacity = prm["eps"], prm["sight"], prm["fcap"], prm["capacity"]
    Q = tab.n_queries
    fld = old.field
    if fld is not None:
        if priors is not None:
            raise ValueError("replan: field and prior(s) exclude each other")
        if not old._owns_field and (fld.stale or goal_rows is not None):
            raise RuntimeError("replan: the caller's goal field is stale or the goal is new: rebuild the field and search anew")
    if goal_rows is not None:
        prm = dict(prm, goal_rows=np.ascontiguousarray(goal_rows, dtype=np.float64))
        if prm["own_goals"]:  # (drops the priors); without: the context's goal decides, set below
            opn.set_goals(prm["goal_rows"], **prm["goal_kw"])
    if priors is not None:
        if not prm["own_goals"]:  # a prior needs the open set's own goal
            prm = dict(prm, own_goals=True)
            opn.set_goals(prm["goal_rows"], **prm["goal_kw"])
        opn.set_prior_list(list(priors))
    if not multi:
        env.set_goal(prm["goal_rows"][0], **prm["goal_kw"])  # (the context's goal may have been moved since the search)
    if fld is not None:  # before the first push: an owned field follows the map and the goal; set_goals dropped it
        foq = old._field_of_query
        if old._owns_field and (fld.stale or goal_rows is not None):
            rows, tol, foq = _distinct_goals(prm["goal_rows"], prm["goal_kw"]["tol_pos"])
            fld.build(rows, tol)
            old._field_of_query = foq
        opn.set_field(fld, foq)
    with contextlib.ExitStack() as always:
        scratch = _own(always, _Scratch())
        kept, sel, imp = (scratch.add(TableFrontier(env, c)) for c in (capacity, fcap, capacity))
        lists = scratch.add(env.alloc_lists(fcap, want_state=True, stride=prm["lists_stride"]))
        if timed:
            executed = _executed(old, tab, roots)
            info = tab.rebase_timed(roots, check_edges=check_edges, allow_wait=wait, avoid=avoid, frontier=kept)
        else:
            info = tab.rebase(roots=roots, check_edges=check_edges, frontier=kept) if multi else \
                tab.rebase(root=roots[0], check_edges=check_edges, frontier=kept)
        _table_check(tab, who, "after the rebase")
        n_kept = info["n_kept"]
        opn.clear()
        opn.push(kept, n_max=n_kept, eps=eps, sight=sight, closed=True)
        if park:
            avoid.park(opn, kept, n_kept)
        rounds, expanded = [0] * Q, [0] * Q
        query = np.zeros(n_kept, np.int32)  # whose the kept rows are: the forced chunks are counted per query
        if multi and n_kept and tab.query_ptr():
            query = tab._read(tab.query_ptr(), np.int32, tab.stats()[0])[kept.id.download(np.int32, (n_kept,))]
        total = 0
        for first in range(0, n_kept, max(fcap, 1)):
            n = min(fcap, n_kept - first)
            _round(env, tab, opn, avoid, kept.rows(first, n), imp, lists, n, prm, wait, park)
            total += 1
            per = np.bincount(query[first:first + n], minlength=Q)
            for q in range(Q):
                if per[q]:
                    rounds[q] += 1
                    expanded[q] += int(per[q])
        status, res, total = _search_loop(env, who, multi, tab, opn, sel, imp, lists, prm, total, rounds, expanded, avoid)
        new = type(old)._of(status, res, tab, opn, rounds, expanded, total, env, prm)
        new.rebase_info = info
        if timed:
            new._executed = executed
        new._hand_field(old)
        old.table = old.open = None  # the new result owns them
        return new


def run_improve(old, multi, eps, prune, max_rounds, max_expand, avoid=None):
    """SearchResult.improve / MultiSearchResult.improve: re-key the open set of `old` for `eps` (pruning what cannot beat
    the costs in hand), then the loop of the search with the new eps.  No rebase, no forced round: the calls of a round
    are those of the search."""
    env, prm, tab, opn = old._env, old._params, old.table, old.open
    _body_current("improve", prm)
    if avoid is not None:
        avoid.set_queries(prm["t0"], prm["radius"], prm["ignore_group"])
    env._flush()
    Q = tab.n_queries
    if not multi:
        env.set_goal(prm["goal_rows"][0], **prm["goal_kw"])  # (the context's goal may have been moved since the search)
    cut = None
    if prune:
        slack, cert = old._certificate()
        found, cost = old._per_query("found"), old._per_query("cost")
        cut = [cost[q] + slack[q] if (found[q] and cert[q]) else math.inf for q in range(Q)]
    rounds, expanded, total = list(old._per_query("rounds")), list(old._per_query("expanded")), old.total_rounds
    if not multi:
        rounds = [total]
    prm = dict(prm, eps=eps)  # what a later replan runs with; the limits below are this call's alone
    run = dict(prm, max_rounds=None if max_rounds is None else total + int(max_rounds),
               max_expand=None if max_expand is None else sum(expanded) + int(max_expand))
    with contextlib.ExitStack() as always:
        scratch = _own(always, _Scratch())
        sel, imp = (scratch.add(TableFrontier(env, c)) for c in (prm["fcap"], prm["capacity"]))
        lists = scratch.add(env.alloc_lists(prm["fcap"], want_state=True, stride=prm["lists_stride"]))
        try:
            info = opn.rekey(eps, cut=cut)
        except _abi.MplxError as e:
            if e.code == _abi.ERR_STATE:
                _table_check(tab, "improve", "before the re-key")
            raise
        status, res, total = _search_loop(env, "improve", multi, tab, opn, sel, imp, lists, run, total, rounds, expanded, avoid)
        new = type(old)._of(status, res, tab, opn, rounds, expanded, total, env, prm)
        new.rebase_info, new._executed, new.rekey_info = old.rebase_info, old._executed, info
        before = old._pruned_at or [math.inf] * Q
        new._pruned_at = [min(a, b) for a, b in zip(before, cut or before)]
        new._hand_field(old)
        old.table = old.open = None  # the new result owns them
        return new


def anytime(result, schedule, max_expand=None, avoid=None):
    """An anytime schedule on one tree: improve `result` (a SearchResult or MultiSearchResult, made with
    any eps) through the eps values of `schedule`, which must not increase.  Stops early once every certified query
    has ratio <= 1 (its cost is proven optimal; with no certified query the schedule runs to its end), or when max_expand
    expansions (all stages and queries together) are spent.  avoid: as improve.  Returns (final_result, stages): per stage
    {"eps", "status", "cost", "lower", "ratio", "certified", "rounds", "expanded"}, each but eps a list per query;
    rounds / expanded are those of the stage alone.  `result` is consumed by the first stage, as improve consumes it."""
    sched = [float(e) for e in schedule]
    if any(b > a for a, b in zip(sched, sched[1:])):
        raise ValueError("anytime: the schedule must be non-increasing")
    stages, spent = [], 0
    for eps in sched:
        if max_expand is not None and spent >= max_expand:
            break
        r0, e0 = list(result._per_query("rounds")), list(result._per_query("expanded"))
        result = result.improve(eps, max_expand=None if max_expand is None else max_expand - spent, avoid=avoid)
        b = result._bound()
        r1, e1 = result._per_query("rounds"), result._per_query("expanded")
        spent += sum(e1) - sum(e0)
        stages.append({"eps": eps, "status": list(result._per_query("status")), "cost": [x["cost"] for x in b],
                       "lower": [x["lower"] for x in b], "ratio": [x["ratio"] for x in b],
                       "certified": [x["certified"] for x in b],
                       "rounds": [a - c for a, c in zip(r1, r0)], "expanded": [a - c for a, c in zip(e1, e0)]})
        cert = [x for x in b if x["certified"]]
        if cert and all(x["ratio"] <= 1.0 for x in cert):
            break
    return result, stages
