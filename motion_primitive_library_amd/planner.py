"""Host-side mirror of the reference's MapPlanner<Dim> (the caller of the hot
path): same method names and argument meaning as

    PlannerBase  reference include/mpl_planner/common/planner_base.h:170-325
    MapPlanner   reference include/mpl_planner/planner/map_planner.h,
                 src/mpl_planner/map_planner.cpp:14-18 (setMapUtil)

The A* itself is the C++ host search inside libmplx.so (csrc/host_planner.hpp);
successors come from the engine context (get_succ on the MI355X).  Tests may
plug another provider through set_provider() -- that is how the CPU oracle is
run under the very same search to pin config C1.
"""
import ctypes as C
import weakref

import numpy as np

from . import _abi
from .env import EnvMap, Waypoint


class MapUtil:
    """MapUtil<Dim> (map_util.h): the map a planner reads, and the operations a user runs on it before planning --
    dilate, freeUnknown, freeAll, the voxel clouds and rayTrace -- on the device.

    The reference's planners share the MapUtil by pointer, so an operation after setMapUtil reaches the next plan() of
    every planner holding it.  Here the operation runs on the engine context of the planner the MapUtil was installed
    in last (its device map is changed in place, nothing is uploaded); every holder's host grid gets the result
    through mplx_planner_set_map, and the device map of any OTHER holder's context the new cells.  A MapUtil no
    planner holds runs on a context of its own on `device`, created on first use; its cells are uploaded once per
    setMap.  There is no CPU implementation: without a GPU the operations raise the engine's no-device error."""

    def __init__(self, dim, device=0):
        self.dim = dim
        self.device = device
        self.origin = self.map_dim = self.cells = self.res = None
        self._holders = []     # weak references to the MapPlanners this MapUtil is installed in, oldest first
        self._version = 0      # bumped by every change of the cells
        self._own = None       # the context of its own (EnvMap), for a MapUtil no planner holds
        self._own_version = -1

    def setMap(self, origin, dim, cells, res):
        self.origin = [float(x) for x in origin]
        self.map_dim = [int(x) for x in dim]
        self.cells = np.ascontiguousarray(cells, dtype=np.int8).ravel()
        self.res = float(res)
        assert self.cells.size == int(np.prod(self.map_dim))
        self._version += 1

    # ---- the reference's operations (map_util.h:136-296)
    def dilate(self, dilate_neighbor):
        """Inflates the obstacles: every cell an offset of `dilate_neighbor` ([n][D] ints) reaches from an occupied cell
        becomes occupied (MapUtil::dilate, map_util.h:220-256)."""
        return self._change(lambda env: env.dilate(dilate_neighbor))

    def freeUnknown(self):
        """Unknown cells (-1) become free (0) (map_util.h:258-276)."""
        return self._change(lambda env: env.freeUnknown())

    def freeAll(self):
        """Every cell becomes free (0) (map_util.h:278-296)."""
        return self._change(lambda env: env.freeAll())

    def getCloud(self):
        """Centres of the occupied cells, (n, D) float64, in the reference's order (x outermost)."""
        return self._env().getCloud()

    def getFreeCloud(self):
        return self._env().getFreeCloud()

    def getUnknownCloud(self):
        return self._env().getUnknownCloud()

    def rayTrace(self, pt1, pt2):
        """MapUtil::rayTrace (map_util.h:117-134): the cells the ray from pt1 to pt2 passes, (n, D) int32 cell
        coordinates in order, without the cells of the end points; stops where the ray leaves the map."""
        env = self._env()
        p1 = np.asarray(pt1, dtype=np.float64).reshape(-1)
        p2 = np.asarray(pt2, dtype=np.float64).reshape(-1)
        n = int(env.ray_trace(p1, p2)["n_cells"][0])
        D = len(self.map_dim)
        if n == 0:
            return np.zeros((0, D), np.int32)
        idx = env.ray_trace(p1, p2, cell_cap=n)["cells"][0].astype(np.int64)
        out = np.empty((n, D), np.int32)
        for i in range(D):
            out[:, i] = idx % self.map_dim[i]
            idx //= self.map_dim[i]
        return out

    # ---- where the operations run
    def _attach(self, planner):
        self._detach(planner)
        self._holders.append(weakref.ref(planner))

    def _detach(self, planner):
        self._holders = [r for r in self._holders if r() is not None and r() is not planner]

    def _planners(self):
        return [p for p in (r() for r in self._holders) if p is not None and p._p]

    def _env(self):
        """The engine context whose device map holds this MapUtil's cells (uploaded first where it does not)."""
        if self.cells is None:
            raise ValueError("MapUtil: setMap first")
        engines = [p for p in self._planners() if p.env is not None]
        if engines:
            p = engines[-1]
            if p._map_version != self._version:
                p.env.setMap(self.origin, self.map_dim, self.cells, self.res)
                p._map_version = self._version
            return p.env
        if self._own is None:
            from .env import EnvMap
            self._own = EnvMap(len(self.map_dim), self.device)
        if self._own_version != self._version:
            self._own.setMap(self.origin, self.map_dim, self.cells, self.res)
            self._own_version = self._version
        return self._own

    def _change(self, op):
        env = self._env()
        new = op(env)  # a NEW array: setMap may have kept a view of the caller's
        self.cells = new
        self._version += 1
        if env is self._own:
            self._own_version = self._version
        for p in self._planners():
            p._map_util_changed(self, device_done=p.env is env)

    def close(self):
        if self._own is not None:
            self._own.close()
            self._own = None

class Trajectory:
    """What the reference's tests read off Trajectory<Dim> (trajectory.h).  With `env` (the engine's EnvMap, as getTraj()
    passes it) sample / evaluate / Jyaw run on the device (include/mplx_traj.h); there is no host implementation."""

    def __init__(self, total_time, J, nodes, actions, cost, end=None, env=None):
        self._T, self._J, self.nodes, self.actions, self.cost, self.end = total_time, J, nodes, actions, cost, end
        self._env = env

    def getWaypoints(self):
        """Rows of 4D+2: the start state of every primitive and the state the last one reaches
        (Trajectory::getWaypoints, trajectory.h)."""
        if self.end is None or len(self.nodes) == 0:
            return np.asarray(self.nodes)
        return np.vstack([self.nodes, self.end[None, :]])

    def getTotalTime(self):
        return self._T

    def J(self, control):
        order = {0x01: 0, 0x03: 1, 0x07: 2, 0x0F: 3}[control & 0x0F]
        return self._J[order]

    def _set(self):
        if self._env is None:
            raise RuntimeError("this Trajectory has no engine env (getTraj() of a planner with provider=None passes one)")
        if len(self.actions) == 0:
            raise RuntimeError("the trajectory has no segment")
        return np.asarray(self.nodes[0], dtype=np.float64), np.asarray(self.actions, dtype=np.int32).reshape(-1, 1)

    def sample(self, N):
        """Trajectory::sample(N): N + 1 Commands at i * (T / N), rows of 4D+3 = pos, vel, acc, jrk, yaw, yaw_dot, t."""
        start, acts = self._set()
        return self._env.traj_sample(start, acts, N=int(N))["samples"][:, 0, :].T.copy()

    def evaluate(self, t, command=True):
        """Trajectory::evaluate at time t: the Command (4D+3 values) or, command=False, the Waypoint's pos, vel, acc,
        jrk, yaw (4D+1 values)."""
        from .env import TRAJ_COMMAND, TRAJ_WAYPOINT
        start, acts = self._set()
        r = self._env.traj_sample(start, acts, times=[float(t)], form=TRAJ_COMMAND if command else TRAJ_WAYPOINT)
        row = r["samples"][:, 0, 0]
        return row.copy() if command else row[:4 * self._env.dim + 1].copy()

    def Jyaw(self):
        start, acts = self._set()
        return float(self._env.traj_info(start, acts)["effort"][4, 0])

    def getSegmentTimes(self):
        """Trajectory::getSegmentTimes: the differences of the accumulated segment times (taus by sequential addition)."""
        if self._env is None:
            raise RuntimeError("this Trajectory has no engine env")
        taus = [0.0]
        for _ in range(len(self.actions)):
            taus.append(float(self._env._p.dt) + taus[-1])
        return [taus[i + 1] - taus[i] for i in range(len(taus) - 1)]


class MapPlanner:
    def __init__(self, dim, device=0, verbose=False, provider=None):
        """provider=None: successors from the HIP engine on `device` (the product
        path; needs a GPU).  provider=(single_fn_ptr, batch_fn_ptr, user_ptr):
        raw C hooks of another env implementation (tests: the CPU oracle)."""
        self.dim = dim
        self._L = _abi.lib()
        p = C.c_void_p()
        rc = self._L.mplx_planner_create(dim, C.byref(p))
        if rc != 0:
            raise _abi.MplxError(rc, "mplx_planner_create failed")
        self._p = p
        self._cfg = _abi.PlannerConfig()
        # nodes per device launch: the result does not depend on it (get_succ is a pure function), the speed does
        self._cfg.control, self._cfg.max_expand, self._cfg.batch = 0x03, -1, (64 if provider is None else 1)
        self._cfg.dt, self._cfg.w, self._cfg.v_max, self._cfg.epsilon = 1.0, 10.0, -1.0, 1.0
        self._cfg.tol_pos, self._cfg.tol_vel, self._cfg.tol_acc, self._cfg.tol_yaw = 0.5, -1.0, -1.0, -1.0
        self.env = None
        self._keep = provider
        self._map_util = None
        self._map_version = -1  # the MapUtil version this planner's device map holds
        self._search_radius = None
        self._potential_radius, self._potential_range, self._pow = None, None, 1.0
        self._traj = None
        if provider is None:
            self.env = EnvMap(dim, device)
            self._check(self._L.mplx_planner_attach_ctx(self._p, self.env._ctx))
        else:
            single, batched, user = provider
            self._check(self._L.mplx_planner_set_provider(self._p, single, batched, user))
        self._summary = None

    def _check(self, rc):
        if rc != 0:
            msg = self._L.mplx_planner_last_error(self._p)
            raise _abi.MplxError(rc, msg.decode() if msg else "?")

    def close(self):
        if self._p:
            self._L.mplx_planner_destroy(self._p)
            self._p = None
        if self.env is not None:
            self.env.close()
            self.env = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- MapPlanner / PlannerBase setters (same names as the reference)
    def setMapUtil(self, map_util):
        if self._map_util is not None and self._map_util is not map_util:
            self._map_util._detach(self)
        self._map_util = map_util
        map_util._attach(self)  # its dilate / freeUnknown / freeAll run on this planner's context from now on
        d = (C.c_int32 * 3)(*(map_util.map_dim + [1] * (3 - len(map_util.map_dim))))
        o = (C.c_double * 3)(*(map_util.origin + [0.0] * (3 - len(map_util.origin))))
        self._check(self._L.mplx_planner_set_map(self._p, map_util.cells.ctypes.data, d, o, map_util.res))
        if self.env is not None:
            self.env.setMap(map_util.origin, map_util.map_dim, map_util.cells, map_util.res)
        self._map_version = map_util._version

    def _map_util_changed(self, mu, device_done):
        """An operation of the MapUtil this planner holds changed its cells: the host grid (start / goal tests) gets
        them; the device map too, unless the operation ran on this planner's own context."""
        d = (C.c_int32 * 3)(*(mu.map_dim + [1] * (3 - len(mu.map_dim))))
        o = (C.c_double * 3)(*(mu.origin + [0.0] * (3 - len(mu.origin))))
        self._check(self._L.mplx_planner_set_map(self._p, mu.cells.ctypes.data, d, o, mu.res))
        if self.env is not None and not device_done:
            self.env.setMap(mu.origin, mu.map_dim, mu.cells, mu.res)
        self._map_version = mu._version

    def setU(self, U):
        U = np.ascontiguousarray(U, dtype=np.float64)
        self._check(self._L.mplx_planner_set_controls(self._p, U.ctypes.data, U.shape[0], U.shape[1]))
        if self.env is not None:
            self.env.set_u(U)

    def _env(self, name, v):
        if self.env is not None:
            getattr(self.env, name)(v)

    def setVmax(self, v): self._cfg.v_max = float(v); self._env("set_v_max", v)
    def setAmax(self, a): self._env("set_a_max", a)
    def setJmax(self, j): self._env("set_j_max", j)
    def setYawmax(self, y): self._env("set_yaw_max", y)
    def setDt(self, dt): self._cfg.dt = float(dt); self._env("set_dt", dt)
    def setW(self, w): self._cfg.w = float(w); self._env("set_w", w)
    def setWyaw(self, w): self._env("set_wyaw", w)
    def setEpsilon(self, eps): self._cfg.epsilon = float(eps)
    def setMaxNum(self, n): self._cfg.max_expand = int(n)

    def setTmax(self, t):
        """PlannerBase::setTmax (planner_base.h:203-205).  Kept and, as in the reference's MapPlanner, without effect on the
        search: t_max is only read by env_base::is_goal (env_base.h:24), which env_map::is_goal (env_map.h:25-45) overrides
        without it."""
        self._t_max = float(t)

    def setTol(self, tol_pos, tol_vel=-1.0, tol_acc=-1.0):
        self._cfg.tol_pos, self._cfg.tol_vel, self._cfg.tol_acc = float(tol_pos), float(tol_vel), float(tol_acc)

    # ---- MapPlanner's map preprocessing and iterative planning (map_planner.h:25-62, map_planner.cpp:46-95,
    #      246-283, 394-430); the kernels are the engine's (EnvMap.updatePotentialMap / setSearchRegion)
    def setSearchRadius(self, r): self._search_radius = [float(x) for x in r]
    def setPotentialRadius(self, r): self._potential_radius = [float(x) for x in r]
    def setPotentialMapRange(self, r): self._potential_range = [float(x) for x in r]
    def setPotentialWeight(self, w): self._env("set_potential_weight", w)
    def setGradientWeight(self, w): self._env("set_gradient_weight", w)

    def setSearchRegion(self, path, dense=False):
        """Cells within the search radius of `path` ([n][D] positions) become the only traversable ones."""
        if self._search_radius is None:
            raise ValueError("setSearchRadius first")
        return self.env.setSearchRegion(np.asarray(path, dtype=np.float64)[:, :self.dim], self._search_radius, dense)

    def updatePotentialMap(self, pos):
        """Rewrites the MapUtil's map with the potential field around the obstacles (map_planner.cpp:246-283, 387)
        and installs it as the env's potential map."""
        if self._potential_radius is None:
            raise ValueError("setPotentialRadius first")
        new_map = self.env.updatePotentialMap(pos, self._potential_radius, self._potential_range, self._pow)
        mu = self._map_util
        mu.cells = new_map
        mu._version += 1
        self._map_version = mu._version
        d = (C.c_int32 * 3)(*(mu.map_dim + [1] * (3 - len(mu.map_dim))))
        o = (C.c_double * 3)(*(mu.origin + [0.0] * (3 - len(mu.origin))))
        self._check(self._L.mplx_planner_set_map(self._p, mu.cells.ctypes.data, d, o, mu.res))
        return new_map

    def iterativePlan(self, start, goal, raw_traj, max_num):
        """MapPlanner::iterativePlan (map_planner.cpp:394-430): re-plan inside the tunnel around the previous
        trajectory until the cost stops changing."""
        traj = raw_traj
        prev_cost = 0.0
        for _ in range(int(max_num)):
            self.setSearchRegion(traj.getWaypoints()[:, :self.dim], False)
            if not self.plan(start, goal):
                return False
            traj = self.getTraj()
            if prev_cost == self.getTrajCost():
                break
            prev_cost = self.getTrajCost()
        return True

    def setBatch(self, n):
        """Nodes per device launch (1 = the reference's one-node-at-a-time loop; default 64 on the engine)."""
        self._cfg.batch = int(n)

    # ---- PlannerBase::plan
    def plan(self, start, goal):
        self._cfg.control = int(start.control)
        self._cfg.goal_control = int(goal.control) if goal.control else 0  # env_base.h:47 hashes the goal with its own flags
        if self.env is not None:
            self.env.set_control(start.control)
            self.env._flush()
        self._check(self._L.mplx_planner_configure(self._p, C.byref(self._cfg)))
        s = np.ascontiguousarray(start.to_row(), dtype=np.float64)
        g = np.ascontiguousarray(goal.to_row(), dtype=np.float64)
        out = _abi.PlanSummary()
        self._check(self._L.mplx_planner_plan(self._p, s.ctypes.data, g.ctypes.data, C.byref(out)))
        self._summary = out
        return bool(out.ok)

    def summary(self):
        o = self._summary
        return {k: getattr(o, k) for k in ("ok", "expansions", "closed", "opened", "nodes", "device_launches",
                                           "pairs", "cost", "total_time", "segments")} | {
            "J": list(o.J), "state_mismatches": o.state_mismatches}

    # ---- incremental re-planning (PlannerBase::setLPAstar, MapPlanner::getLinkedNodes / updateBlockedNodes /
    #      updateClearedNodes, StateSpace::getSubStateSpace): the state space outlives plan()
    def setLPAstar(self, on=True):
        self._check(self._L.mplx_planner_set_lpastar(self._p, 1 if on else 0))

    def reset(self):
        self._check(self._L.mplx_planner_reset(self._p))

    def getLinkedNodes(self, want_points=True):
        """(Re)builds the voxel -> edge table; returns (points [n][D] or None, number of cells, number of entries)."""
        n, cells, entries = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._L.mplx_planner_linked_nodes(self._p, None, 0, C.byref(n), C.byref(cells), C.byref(entries)))
        pts = None
        if want_points:
            pts = np.empty((max(n.value, 1), self.dim), dtype=np.float64)
            self._check(self._L.mplx_planner_linked_nodes(self._p, pts.ctypes.data, n.value, C.byref(n), C.byref(cells), C.byref(entries)))
            pts = pts[:n.value]
        return pts, cells.value, entries.value

    def _edit_map(self, cells, value):
        """The caller's side of a map edit (the reference's test edits its MapUtil and calls setMap): the planner's host
        copy and the device map get the new cells."""
        mu = self._map_util
        cells = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, self.dim)
        idx = cells[:, 0].astype(np.int64)
        mul = 1
        for i in range(1, self.dim):
            mul *= mu.map_dim[i - 1]
            idx = idx + mul * cells[:, i]
        # O(edited cells) everywhere: the MapUtil's array in place (copied once, only if it cannot be written), the
        # planner's host copy (start / goal tests) through mplx_planner_edit_map, the device through mplx_edit_map
        if not mu.cells.flags.writeable:
            mu.cells = mu.cells.copy()
        mu.cells[idx] = value
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        val = np.full(idx.size, value, dtype=np.int8)
        self._check(self._L.mplx_planner_edit_map(self._p, idx.ctypes.data, val.ctypes.data, idx.size))
        if self.env is not None:
            self.env.editMap(idx, val)
        return cells

    def updateBlockedNodes(self, cells, edit_map=True):
        cells = self._edit_map(cells, 100) if edit_map else np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, self.dim)
        self._check(self._L.mplx_planner_update_blocked_nodes(self._p, cells.ctypes.data, cells.shape[0]))

    def updateClearedNodes(self, cells, edit_map=True):
        cells = self._edit_map(cells, 0) if edit_map else np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, self.dim)
        if self.env is not None:
            self.env._flush()
        self._check(self._L.mplx_planner_update_cleared_nodes(self._p, cells.ctypes.data, cells.shape[0]))

    def getSubStateSpace(self, time_step):
        self._check(self._L.mplx_planner_sub_state_space(self._p, int(time_step)))

    def setEdgeProvider(self, fn_ptr, user_ptr):
        """Tests: another implementation of the batched edge re-validation (the CPU oracle's)."""
        self._check(self._L.mplx_planner_set_edge_provider(self._p, fn_ptr, user_ptr))

    def setPriorTrajectory(self, other, potential=None, potential_weight=None, gradient_weight=None):
        """PlannerBase::setPriorTrajectory: the last trajectory of another planner (still open) guides this one's
        search; None clears it.  Set this planner's map, v_max, w and dt first -- and the potential map, if any
        (env_map::set_prior_trajectory reads potential_map_, env_map.h:197-216): with the engine's own env the values
        of the cells the prior passes through are read from the device's potential map; a planner on another
        provider passes its host copy as `potential` with the two weights."""
        self._check(self._L.mplx_planner_configure(self._p, C.byref(self._cfg)))  # (v_max, w, dt reach the search)
        if other is not None and (potential is not None or (self.env is not None and self.env.has_potential)):
            if potential is not None:
                potential = np.ascontiguousarray(potential, dtype=np.int8).ravel()
                pw, gw = float(potential_weight), float(gradient_weight or 0.0)
                ptr = potential.ctypes.data
            else:
                self.env._flush()
                (pw, gw), ptr = self.env.potential_weights(), None
            self._check(self._L.mplx_planner_set_prior_trajectory_potential(self._p, other._p, ptr, C.c_double(pw), C.c_double(gw)))
            return
        self._check(self._L.mplx_planner_set_prior_trajectory(self._p, other._p if other is not None else None))

    def useDeviceHeuristic(self, on=True):
        """The heuristic of new nodes from the `heur` row the expansion launches write (mplx_set_goal) instead of the
        search's own evaluation: same search, see mplx_planner_use_device_heuristic."""
        self._check(self._L.mplx_planner_use_device_heuristic(self._p, 1 if on else 0))

    def setHeurIgnoreDynamics(self, ignore=True, robust=False):
        """PlannerBase::setHeurIgnoreDynamics (planner_base.h; env_base::cal_heur): ignore=True -- the default heuristic
        w * Linf / v_max.  ignore=False -- the cost of the unconstrained connection from the state to the goal state,
        minimised over the arrival time (include/mplx_heur.h): robust=False is the REFERENCE mode, what the reference
        returns expression for expression (VEL and ACC state spaces; not admissible), robust=True the
        ROBUST mode, the true minimum (VEL, ACC and JRK; never below the default).  For A* and LPA*; a prior trajectory
        excludes both."""
        mode = _abi.HEUR_DEFAULT if ignore else (_abi.HEUR_ROBUST if robust else _abi.HEUR_REFERENCE)
        self._check(self._L.mplx_planner_set_heur_dynamics(self._p, mode))

    def timing(self):
        """Where the wall time of the last plan() went (ms) and what its relaxation loop did (mplx_plan_timing)."""
        t = _abi.PlanTiming()
        self._check(self._L.mplx_planner_timing(self._p, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _abi.PlanTiming._fields_}

    def getCloseSet(self):
        n = C.c_int32()
        self._check(self._L.mplx_planner_closed_set(self._p, None, 0, C.byref(n)))
        pts = np.empty((n.value, self.dim), dtype=np.float64)
        self._check(self._L.mplx_planner_closed_set(self._p, pts.ctypes.data, n.value, C.byref(n)))
        return pts

    def getOpenStates(self):
        """Full states (rows of 4D+2) of the open set of the last plan (PlannerBase::getOpenSet gives positions)."""
        n = C.c_int32()
        self._check(self._L.mplx_planner_open_set(self._p, None, 0, C.byref(n)))
        f = 4 * self.dim + 2
        rows = np.empty((n.value, f), dtype=np.float64)
        self._check(self._L.mplx_planner_open_set(self._p, rows.ctypes.data, n.value, C.byref(n)))
        return rows

    def getTraj(self):
        o = self._summary
        f = 4 * self.dim + 2
        nodes = np.empty((max(o.segments, 1), f), dtype=np.float64)
        acts = np.empty(max(o.segments, 1), dtype=np.int32)
        self._check(self._L.mplx_planner_trajectory(self._p, nodes.ctypes.data, acts.ctypes.data, max(o.segments, 1)))
        end = np.empty(f, dtype=np.float64)
        if o.ok and o.segments > 0:
            self._check(self._L.mplx_planner_trajectory_end(self._p, end.ctypes.data))
        else:
            end = None
        return Trajectory(o.total_time, list(o.J), nodes[:o.segments], acts[:o.segments], o.cost, end, env=self.env)

    def getTrajCost(self):
        return self._summary.cost

    def checkTraj(self):
        """The last plan's trajectory -- its start state and one control index per segment -- walked again on the map
        the device holds NOW (EnvMap.rollout): (status, steps, cost).  status SLOT_FINITE and cost == getTrajCost()
        while the trajectory is still valid; after a map edit the slot status of the first segment that is not
        (SLOT_BLOCKED, ...), the number of segments before it, and +inf."""
        if self.env is None:
            raise RuntimeError("checkTraj needs the engine's own env (provider=None)")
        traj = self.getTraj()
        if len(traj.actions) == 0:
            raise RuntimeError("checkTraj: the last plan has no trajectory")
        r = self.env.rollout(np.asarray(traj.nodes[0], dtype=np.float64), np.asarray(traj.actions, dtype=np.int32).reshape(-1, 1),
                             want_end=False)
        return int(r["status"][0]), int(r["steps"][0]), float(r["cost"][0])

    def traverseTraj(self):
        """env_map::traverse_trajectory of the last plan's trajectory on the maps the device holds NOW
        (EnvMap.traj_traverse): (cost, stop_sample) -- 0.0 or the potential sum and -1 while the trajectory is free,
        +inf and the index of the sample that hit an occupied cell or left the map after a map edit."""
        if self.env is None:
            raise RuntimeError("traverseTraj needs the engine's own env (provider=None)")
        traj = self.getTraj()
        if len(traj.actions) == 0:
            raise RuntimeError("traverseTraj: the last plan has no trajectory")
        r = self.env.traj_traverse(np.asarray(traj.nodes[0], dtype=np.float64), np.asarray(traj.actions, dtype=np.int32).reshape(-1, 1))
        return float(r["cost"][0]), int(r["stop_sample"][0])


class TrajSolver:
    """TrajSolver<Dim> (reference include/mpl_traj_solver/traj_solver.h): the minimum-velocity / acceleration / jerk
    polynomial through waypoints, solved on the device (include/mplx_solve.h; EnvMap.solve_traj is the batched form).
    control: of the two ends, VEL / ACC / JRK; yaw_control: VEL.  env: the EnvMap to solve on (one is made otherwise)."""

    def __init__(self, dim, control, yaw_control=0x01, env=None, device=0):
        from .env import _solve_order
        _solve_order(control)
        self.dim, self.control, self.yaw_control = int(dim), int(control), int(yaw_control)
        self._env, self._own_env = (env, False) if env is not None else (EnvMap(dim, device), True)
        self._waypoints, self._flags, self._path = [], None, np.zeros((0, dim))
        self._dts, self._v = [], 1.0

    def close(self):
        if self._own_env and self._env is not None:
            self._env.close()
        self._env = None

    def setWaypoints(self, ws):
        """Waypoints with their own control flags (use_pos / use_vel / use_acc = the low bits of Waypoint.control)."""
        self._waypoints = [Waypoint(self.dim, w.control, w.pos, w.vel, w.acc, w.jrk, w.yaw, w.t) for w in ws]
        self._path = np.array([w.pos for w in self._waypoints], dtype=np.float64).reshape(-1, self.dim)
        self._flags = np.array([int(w.control) & 0x07 for w in self._waypoints], dtype=np.uint8)

    def setV(self, v):
        self._v = float(v)

    def setDts(self, dts):
        self._dts = [float(x) for x in dts]

    def setPath(self, path):
        """Positions only: interior waypoints are Control::VEL, the ends the solver's control; vel / acc / jrk / yaw are
        zeroed as the reference does (traj_solver.h:55-70)."""
        self._path = np.asarray(path, dtype=np.float64).reshape(-1, self.dim)
        self._waypoints = [Waypoint(self.dim, 0x01, p) for p in self._path]
        if self._waypoints:
            self._waypoints[0].control = self._waypoints[-1].control = self.control
        self._flags = None

    def solve(self):
        """Returns the PolyTrajSet of the one problem (status, coefficients(), sample(), info(), traverse())."""
        W = len(self._waypoints)
        rows = np.zeros((self._env.n_fields, max(W, 2), 1))
        for w, wp in enumerate(self._waypoints):
            rows[:, w, 0] = wp.to_row()
        given = len(self._dts) + 1 == W  # traj_solver.h:74
        dts = np.asarray(self._dts, dtype=np.float64).reshape(-1, 1) if given and W >= 2 else None
        flags = None
        if self._flags is not None:
            flags = np.zeros((max(W, 2), 1), np.uint8)
            flags[:W, 0] = self._flags
        out = self._env.solve_traj(rows, n_wp=[W], dts=dts, v=self._v, control=self.control, wp_flags=flags,
                                   yaw_control=self.yaw_control)
        if not given and out.status[0] == 0:
            self._dts = [float(x) for x in out.dts()[:W - 1, 0]]
        return out

    def getPath(self):
        return self._path.copy()

    def getWaypoints(self):
        return list(self._waypoints)

    def getDts(self):
        return list(self._dts)
