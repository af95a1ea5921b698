"""Host-side mirror of the reference's env_map<Dim> for the one path this
package replaces: successor expansion.

Names and argument meaning follow the reference so that code (and tests)
written against MPL read the same:

    reference                                   here
    ----------------------------------------    -------------------------------
    MapUtil<Dim>::setMap       map_util.h:84    EnvMap.setMap(origin, dim, map, res)
    env_base::set_u            env_base.h:234   EnvMap.set_u(U)
    env_base::set_v_max ...    env_base.h:237+  EnvMap.set_v_max(v) ...
    env_base::set_dt/w/wyaw    env_base.h:264+  EnvMap.set_dt / set_w / set_wyaw
    env_map::set_potential_map env_map.h:181    EnvMap.set_potential_map(map)
    env_base::set_search_region env_base.h:301  EnvMap.set_search_region(mask)
    env_map::get_succ          env_map.h:147    EnvMap.get_succ(curr) -> (succ, cost, action)

plus the batched forms that are the point of the engine: EnvMap.expand(nodes)
(host arrays) and EnvMap.expand_resident(frontier, slots) (HBM-resident).

Everything below the method bodies is the C ABI of include/mplx.h; numpy is
used only to own host buffers.  No CPU implementation exists here.
"""
import ctypes as C

import numpy as np

from . import _abi
# the device allocations and output rows (rows.py) and the trajectory sets (poly.py), under the names they always had here
from .rows import (DeviceArray, DeviceArrayView, _alloc, _device_ptr, Rollouts, Rays, TrajInfo, TrajSamples,  # noqa: F401
                   TrajTraverse, SolveOut, LoadOut, PolyLimits, LambdaRows, Conflicts, ConflictResult)
from .poly import PolyTrajSet, ShortcutResult, _conflict_in, _conflict_steps, _conflict_host_out  # noqa: F401

# Control::Control (reference include/mpl_basis/control.h:10-20)
VEL, ACC, JRK, SNP = 0x01, 0x03, 0x07, 0x0F
VELxYAW, ACCxYAW, JRKxYAW, SNPxYAW = 0x11, 0x13, 0x17, 0x1F

SLOT_SKIP_SAME, SLOT_FINITE, SLOT_BLOCKED, SLOT_SKIP_DYN = 0, 1, 2, 3
ROLLOUT_BAD_ACTION, ROLLOUT_HEADING_BAND = _abi.ROLLOUT_BAD_ACTION, _abi.ROLLOUT_HEADING_BAND  # include/mplx_rollout.h
RAY_LEFT_MAP, RAY_HIT, RAY_BAD, RAY_TRUNCATED = _abi.RAY_LEFT_MAP, _abi.RAY_HIT, _abi.RAY_BAD, _abi.RAY_TRUNCATED  # include/mplx_ray.h
FLAG_GOAL_BLOCKED = _abi.FLAG_GOAL_BLOCKED
TRAJ_EMPTY, TRAJ_BAD_ACTION, TRAJ_BAD = _abi.TRAJ_EMPTY, _abi.TRAJ_BAD_ACTION, _abi.TRAJ_BAD  # include/mplx_traj.h
TRAJ_COMMAND, TRAJ_WAYPOINT = _abi.TRAJ_COMMAND, _abi.TRAJ_WAYPOINT
SOLVE_EMPTY, SOLVE_BAD_TIME, SOLVE_SINGULAR = _abi.SOLVE_EMPTY, _abi.SOLVE_BAD_TIME, _abi.SOLVE_SINGULAR  # include/mplx_solve.h
LIMITS_REFERENCE, LIMITS_ALL_ROOTS = _abi.LIMITS_REFERENCE, _abi.LIMITS_ALL_ROOTS  # include/mplx_limits.h
EXCEED_VEL, EXCEED_ACC, EXCEED_JRK = _abi.EXCEED_VEL, _abi.EXCEED_ACC, _abi.EXCEED_JRK
SHORTCUT_BAD_CHAIN = _abi.SHORTCUT_BAD_CHAIN
USE_POS, USE_VEL, USE_ACC = _abi.USE_POS, _abi.USE_VEL, _abi.USE_ACC
SCALE_REFERENCE, SCALE_ROBUST = _abi.SCALE_REFERENCE, _abi.SCALE_ROBUST  # include/mplx_scale.h
LAMBDA_BAD_POINTS, LAMBDA_NOT_POSITIVE, LAMBDA_MAX_SEGS = _abi.LAMBDA_BAD_POINTS, _abi.LAMBDA_NOT_POSITIVE, _abi.LAMBDA_MAX_SEGS
CONFLICT_PARK, CONFLICT_GONE, CONFLICT_BAD_INPUT = _abi.CONFLICT_PARK, _abi.CONFLICT_GONE, _abi.CONFLICT_BAD_INPUT  # include/mplx_conflict.h


class Waypoint:
    """Waypoint<Dim> (reference include/mpl_basis/waypoint.h:23-57)."""

    __slots__ = ("dim", "pos", "vel", "acc", "jrk", "yaw", "t", "control")

    def __init__(self, dim, control=0, pos=None, vel=None, acc=None, jrk=None, yaw=0.0, t=0.0):
        self.dim = dim
        self.control = control
        z = np.zeros(dim)
        self.pos = z.copy() if pos is None else np.asarray(pos, dtype=np.float64).copy()
        self.vel = z.copy() if vel is None else np.asarray(vel, dtype=np.float64).copy()
        self.acc = z.copy() if acc is None else np.asarray(acc, dtype=np.float64).copy()
        self.jrk = z.copy() if jrk is None else np.asarray(jrk, dtype=np.float64).copy()
        self.yaw = float(yaw)
        self.t = float(t)

    def to_row(self):
        return np.concatenate([self.pos, self.vel, self.acc, self.jrk, [self.yaw, self.t]])

    @classmethod
    def from_row(cls, dim, control, row):
        d = dim
        return cls(dim, control, row[0:d], row[d:2 * d], row[2 * d:3 * d], row[3 * d:4 * d], row[4 * d],
                   row[4 * d + 1])

    def __repr__(self):
        return "Waypoint(pos=%s, vel=%s, acc=%s, jrk=%s, yaw=%r, t=%r)" % (
            self.pos.tolist(), self.vel.tolist(), self.acc.tolist(), self.jrk.tolist(), self.yaw, self.t)


class Slots:
    """HBM-resident dense successor slots for n_nodes x nU pairs."""

    def __init__(self, env, n_nodes, nU, want_state=True, want_iters=False):
        self.n_nodes, self.nU = int(n_nodes), int(nU)
        self.n_slots = self.n_nodes * self.nU
        self.n_fields = env.n_fields
        n = max(self.n_slots, 1)
        self.status = DeviceArray(env, n)
        self.cost = DeviceArray(env, n * 8)
        self.hash = DeviceArray(env, n * 8)
        self.state = DeviceArray(env, n * 8 * self.n_fields) if want_state else None
        self.iters = DeviceArray(env, n * 4) if want_iters else None

    def c_struct(self):
        s = _abi.Succ()
        s.status, s.cost, s.hash = self.status.ptr, self.cost.ptr, self.hash.ptr
        s.state = self.state.ptr if self.state else None
        s.state_stride = self.n_slots
        s.iters = self.iters.ptr if self.iters else None
        return s

    def download(self):
        out = {
            "status": self.status.download(np.uint8, (self.n_slots,)),
            "cost": self.cost.download(np.float64, (self.n_slots,)),
            "hash": self.hash.download(np.uint64, (self.n_slots,)),
        }
        if self.state:
            out["state"] = self.state.download(np.float64, (self.n_fields, self.n_slots))
        if self.iters:
            out["iters"] = self.iters.download(np.int32, (self.n_slots,))
        return out

    def free(self):
        for b in (self.status, self.cost, self.hash, self.state, self.iters):
            if b is not None:
                b.free()


def _solve_order(control):
    """Smoothing order of a control flag (traj_solver.h:22-27): 0 VEL, 1 ACC, 2 JRK."""
    try:
        return {VEL: 0, ACC: 1, JRK: 2}[int(control) & 0x0F]
    except KeyError:
        raise ValueError("the trajectory solver takes VEL, ACC or JRK controls, got %#x" % int(control))


STATE_ROW_PAD = 0  # default padding between the state rows of Lists, in entries (see Lists.state_stride)


class Lists:
    """HBM-resident per-node successor lists (mplx_succ_lists)."""

    def __init__(self, env, n_nodes, nU, want_state=True, want_iters=False, want_hash=True, stride=None, alloc=None,
                 state_pad=None, want_heur=False, want_flags=False):
        self.n_nodes, self.nU = int(n_nodes), int(nU)
        # entries reserved per node: a multiple of 32 keeps every node's rows on 128-byte lines (and lets the
        # kernel complete the last line of each list instead of leaving a partial-line store)
        self.stride = (self.nU + 31) & ~31 if stride is None else int(stride)
        self.n_slots = self.n_nodes * self.stride
        self.n_fields = env.n_fields
        n = max(self.n_slots, 1)
        self.count = _alloc(env, max(self.n_nodes, 1) * 4, alloc)
        self.action = _alloc(env, n * 4, alloc)
        self.cost = _alloc(env, n * 8, alloc)
        self.hash = _alloc(env, n * 8, alloc) if want_hash else None
        # entries between consecutive state rows (mplx_succ_lists::state_stride): n_slots + state_pad
        self.state_stride = n + (STATE_ROW_PAD if state_pad is None else int(state_pad))
        self._state = _alloc(env, self.state_stride * 8 * self.n_fields, alloc) if want_state else None
        self.iters = _alloc(env, n * 4, alloc) if want_iters else None
        # rows the expansion launch fills for the search (mplx_set_goal): default heuristic, goal flags
        self.heur = _alloc(env, n * 8, alloc) if want_heur else None
        self.flags = _alloc(env, n, alloc) if want_flags else None
        # State rows known to hold +0.0 in every entry (include/mplx.h, mplx_expand_lists_device_z): the rows are
        # zero-filled once here, and EnvMap.expand_lists_resident hands the mask from launch to launch, so that a launch
        # does not store the rows its control can only fill with +0.0.  Whatever else writes into the state rows
        # sets it to 0.  (Synchronised: the buffer may be handed to another context, i.e. another stream, next.)
        self.zero_rows = 0
        if self._state:
            m = C.c_uint32(0)
            s = self.c_struct()
            _abi.check(env._ctx, _abi.lib().mplx_lists_zero_fill(env._ctx, C.byref(s), C.byref(m)))
            _abi.check(env._ctx, _abi.lib().mplx_synchronize(env._ctx))
            self.zero_rows = int(m.value)

    @property
    def state(self):
        return self._state

    @state.setter
    def state(self, buf):
        # another buffer under the same name: nothing is known about its contents (a fresh allocation is not zero)
        self._state = buf
        self.zero_rows = 0

    def c_struct(self):
        s = _abi.SuccLists()
        s.count, s.action, s.cost = self.count.ptr, self.action.ptr, self.cost.ptr
        s.hash = self.hash.ptr if self.hash else None
        s.state = self.state.ptr if self.state else None
        s.state_stride = self.state_stride
        s.iters = self.iters.ptr if self.iters else None
        s.node_stride = self.stride
        s.heur = self.heur.ptr if self.heur else None
        s.flags = self.flags.ptr if self.flags else None
        return s

    def download(self):
        out = {
            "stride": self.stride,
            "count": self.count.download(np.int32, (self.n_nodes,)),
            "action": self.action.download(np.int32, (self.n_slots,)),
            "cost": self.cost.download(np.float64, (self.n_slots,)),
        }
        if self.hash:
            out["hash"] = self.hash.download(np.uint64, (self.n_slots,))
        if self.state:
            st = self.state.download(np.float64, (self.n_fields, self.state_stride))
            out["state"] = np.ascontiguousarray(st[:, :self.n_slots]) if self.state_stride != self.n_slots else st
        if self.iters:
            out["iters"] = self.iters.download(np.int32, (self.n_slots,))
        if self.heur:
            out["heur"] = self.heur.download(np.float64, (self.n_slots,))
        if self.flags:
            out["flags"] = self.flags.download(np.uint8, (self.n_slots,))
        return out

    def download_nodes(self, lo, hi):
        """The lists of nodes [lo, hi) only, as download() would return them for a frontier of hi - lo nodes
        (lets a host with less memory than the device walk a full-size result chunk by chunk)."""
        lo, hi = int(lo), int(hi)
        n, S = hi - lo, self.stride
        out = {
            "stride": S,
            "count": self.count.download(np.int32, (n,), lo * 4),
            "action": self.action.download(np.int32, (n * S,), lo * S * 4),
            "cost": self.cost.download(np.float64, (n * S,), lo * S * 8),
        }
        if self.hash:
            out["hash"] = self.hash.download(np.uint64, (n * S,), lo * S * 8)
        if self.state:
            st = np.empty((self.n_fields, n * S), np.float64)
            for r in range(self.n_fields):
                st[r] = self.state.download(np.float64, (n * S,), (r * self.state_stride + lo * S) * 8)
            out["state"] = st
        if self.iters:
            out["iters"] = self.iters.download(np.int32, (n * S,), lo * S * 4)
        return out

    def free(self):
        for b in (self.count, self.action, self.cost, self.hash, self.state, self.iters, self.heur, self.flags):
            if b is not None:
                b.free()


class PackedLists:
    """HBM-resident packed successor lists (mplx_packed_lists): node k owns entries [offs[k], offs[k+1]) of every
    row, no padding -- the form the multi-GPU all-gather moves and an on-device consumer reads."""

    def __init__(self, env, n_nodes, capacity, want_state=True, want_hash=True, alloc=None):
        self.n_nodes, self.capacity = int(n_nodes), max(int(capacity), 1)
        self.n_fields = env.n_fields
        c = self.capacity
        self.count = _alloc(env, max(self.n_nodes, 1) * 4, alloc)
        self.offs = _alloc(env, (self.n_nodes + 1) * 8, alloc)
        self.action = _alloc(env, c * 4, alloc)
        self.cost = _alloc(env, c * 8, alloc)
        self.hash = _alloc(env, c * 8, alloc) if want_hash else None
        self.state = _alloc(env, c * 8 * self.n_fields, alloc) if want_state else None

    def c_struct(self):
        s = _abi.PackedLists()
        s.count, s.offs, s.action, s.cost = self.count.ptr, self.offs.ptr, self.action.ptr, self.cost.ptr
        s.hash = self.hash.ptr if self.hash else None
        s.state = self.state.ptr if self.state else None
        s.state_stride = self.capacity
        s.capacity = self.capacity
        return s

    def download(self, n_nodes=None):
        n = self.n_nodes if n_nodes is None else int(n_nodes)
        offs = self.offs.download(np.int64, (n + 1,))
        total = int(offs[n])
        out = {"offs": offs, "total": total, "count": self.count.download(np.int32, (n,)),
               "action": self.action.download(np.int32, (total,)), "cost": self.cost.download(np.float64, (total,))}
        if self.hash:
            out["hash"] = self.hash.download(np.uint64, (total,))
        if self.state:
            out["state"] = self.state.download(np.float64, (self.n_fields, self.capacity))[:, :total]
        return out

    def free(self):
        for b in (self.count, self.offs, self.action, self.cost, self.hash, self.state):
            if b is not None:
                b.free()


def pack_host_lists(lists, n_nodes):
    """Host-side restatement of mplx_pack_lists_device on downloaded lists (tests, CPU stand-ins)."""
    S = int(lists["stride"])
    cnt = np.asarray(lists["count"][:n_nodes], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    src = (np.repeat(np.arange(n_nodes, dtype=np.int64) * S - offs[:-1], cnt) + np.arange(offs[-1], dtype=np.int64))
    out = {"offs": offs, "total": int(offs[-1]), "count": cnt.astype(np.int32)}
    for k in ("action", "cost", "hash"):
        if lists.get(k) is not None:
            out[k] = lists[k][src]
    if lists.get("state") is not None:
        out["state"] = lists["state"][:, src]
    return out


def lists_from_dense(dense, n_nodes, nU):
    """Dense slots -> the per-node list layout of mplx_succ_lists (host-side
    helper for tests and examples).  Unused tail entries are left as zeros."""
    st = dense["status"].reshape(n_nodes, nU)
    emit = (st == 1) | (st == 2)
    count = emit.sum(axis=1).astype(np.int32)
    out = {"count": count, "action": np.zeros(n_nodes * nU, np.int32), "cost": np.zeros(n_nodes * nU, np.float64),
           "hash": np.zeros(n_nodes * nU, np.uint64)}
    if dense.get("state") is not None:
        out["state"] = np.zeros_like(dense["state"])
    if dense.get("iters") is not None:
        out["iters"] = np.zeros(n_nodes * nU, np.int32)
    for k in range(n_nodes):
        ci = np.nonzero(emit[k])[0]
        src = k * nU + ci
        dst = k * nU + np.arange(ci.size)
        out["action"][dst] = ci
        out["cost"][dst] = dense["cost"][src]
        out["hash"][dst] = dense["hash"][src]
        if "state" in out:
            out["state"][:, dst] = dense["state"][:, src]
        if "iters" in out:
            out["iters"][dst] = dense["iters"][src]
    return out


class EnvMap:
    """env_map<Dim> whose get_succ runs on the MI355X (reference env_map.h)."""

    def __init__(self, dim, device=0):
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        self.dim = dim
        self._ctx = None
        L = _abi.lib()
        ctx = C.c_void_p()
        rc = L.mplx_create(dim, device, C.byref(ctx))
        if rc != _abi.OK:
            msg = L.mplx_last_error(None)
            raise _abi.MplxError(rc, msg.decode() if msg else "?")
        self._ctx = ctx
        # env_base.h:368-392 / env_map.h:294-296 defaults
        self._p = _abi.Params()
        self._p.control = ACC
        self._p.dt, self._p.w, self._p.wyaw = 1.0, 10.0, 1.0
        self._p.v_max = self._p.a_max = self._p.j_max = self._p.yaw_max = -1.0
        self._p.potential_weight, self._p.gradient_weight = 0.1, 0.0
        self.has_potential = False
        self._dirty = True
        self.nU = 0
        self.map_dim = None
        self._geometry = None  # (dim, origin, res) of the map the context holds

    # ---- lifetime
    def close(self):
        if self._ctx:
            _abi.lib().mplx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def n_fields(self):
        return 4 * self.dim + 2

    def device_info(self):
        buf = C.create_string_buffer(256)
        cus = C.c_int32()
        _abi.check(self._ctx, _abi.lib().mplx_device_info(self._ctx, buf, 256, C.byref(cus)))
        return buf.value.decode(), cus.value

    # ---- map (MapUtil<Dim>::setMap, map_util.h:84-90)
    def setMap(self, origin, dim, cells, res):
        cells = np.ascontiguousarray(cells, dtype=np.int8).ravel()
        d = (C.c_int32 * 3)(*([int(x) for x in dim] + [1] * (3 - len(dim))))
        o = (C.c_double * 3)(*([float(x) for x in origin] + [0.0] * (3 - len(origin))))
        n = int(np.prod([int(x) for x in dim]))
        if cells.size != n:
            raise ValueError("map has %d cells, dim says %d" % (cells.size, n))
        geometry = ([int(x) for x in dim], [float(x) for x in origin], float(res))
        _abi.check(self._ctx, _abi.lib().mplx_set_map(self._ctx, cells.ctypes.data, d, o, float(res)))
        if geometry != self._geometry:
            self.has_potential = False  # mplx_set_map drops the potential map (and the region) of another geometry
        self._geometry = geometry
        self.map_dim = [int(x) for x in dim]
        self._ncell = n

    def editMap(self, cell_index, values):
        """A few cells of the map already on the device take new values (mplx_edit_map): cell_index = x + dim0 * (y +
        dim1 * z) as MapUtil::getIndex numbers them."""
        idx = np.ascontiguousarray(cell_index, dtype=np.int64).ravel()
        val = np.ascontiguousarray(values, dtype=np.int8).ravel()
        if val.size == 1 and idx.size > 1:
            val = np.full(idx.size, val[0], dtype=np.int8)
        if idx.size != val.size:
            raise ValueError("editMap: %d indices, %d values" % (idx.size, val.size))
        _abi.check(self._ctx, _abi.lib().mplx_edit_map(self._ctx, idx.ctypes.data, val.ctypes.data, idx.size))

    def read_cells(self, cell_index, potential=False):
        """Values of a few cells of the map (or the potential map) the device holds (mplx_read_cells)."""
        idx = np.ascontiguousarray(cell_index, dtype=np.int64).ravel()
        out = np.empty(idx.size, dtype=np.int8)
        _abi.check(self._ctx, _abi.lib().mplx_read_cells(self._ctx, 1 if potential else 0, idx.ctypes.data, idx.size, out.ctypes.data))
        return out

    def potential_weights(self):
        return float(self._p.potential_weight), float(self._p.gradient_weight)

    def map_upload_bytes(self):
        """Host -> device bytes the map calls of this context have moved so far (mplx_map_upload_bytes)."""
        b = C.c_uint64(0)
        _abi.check(self._ctx, _abi.lib().mplx_map_upload_bytes(self._ctx, C.byref(b)))
        return int(b.value)

    # ---- env_base / env_map setters
    def set_control(self, control):
        """The control flag of the search (Waypoint::control of the start node)."""
        self._p.control = int(control)
        self._dirty = True

    def set_u(self, U):
        U = np.ascontiguousarray(U, dtype=np.float64)
        if U.ndim != 2:
            raise ValueError("U must be [nU][udim]")
        _abi.check(self._ctx, _abi.lib().mplx_set_controls(self._ctx, U.ctypes.data, U.shape[0], U.shape[1]))
        self.nU = U.shape[0]
        self._U_host = U.copy()  # (what SearchResult.as_prior hands to a later search as the prior's control table)

    def _setp(self, name, v):
        setattr(self._p, name, float(v))
        self._dirty = True

    def set_v_max(self, v): self._setp("v_max", v)
    def set_a_max(self, a): self._setp("a_max", a)
    def set_j_max(self, j): self._setp("j_max", j)
    def set_yaw_max(self, y): self._setp("yaw_max", y)
    def set_dt(self, dt): self._setp("dt", dt)
    def set_w(self, w): self._setp("w", w)
    def set_wyaw(self, w): self._setp("wyaw", w)
    def set_potential_weight(self, w): self._setp("potential_weight", w)
    def set_gradient_weight(self, w): self._setp("gradient_weight", w)

    def set_potential_map(self, cells):
        self.has_potential = not (cells is None or len(cells) == 0)
        if not self.has_potential:
            _abi.check(self._ctx, _abi.lib().mplx_set_potential(self._ctx, None))
            return
        cells = np.ascontiguousarray(cells, dtype=np.int8).ravel()
        if cells.size != self._ncell:
            raise ValueError("potential map size mismatch")
        _abi.check(self._ctx, _abi.lib().mplx_set_potential(self._ctx, cells.ctypes.data))

    def set_search_region(self, mask):
        if mask is None or len(mask) == 0:
            _abi.check(self._ctx, _abi.lib().mplx_set_region(self._ctx, None))
            return
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8).ravel()
        if mask.size != self._ncell:
            raise ValueError("search region size mismatch")
        _abi.check(self._ctx, _abi.lib().mplx_set_region(self._ctx, mask.ctypes.data))

    # ---- MapPlanner-level map preprocessing on the device (map_planner.cpp:46-95, 246-391)
    def updatePotentialMap(self, pos, radius, range_=None, power=1.0):
        """MapPlanner::updatePotentialMap: stamps the potential field into the device map (which it also
        installs as the potential map, as the reference does) and returns the new int8 map."""
        D = len(self.map_dim)
        p = (C.c_double * 3)(*([float(x) for x in pos] + [0.0] * (3 - D)))
        r = (C.c_double * 3)(*([float(x) for x in radius] + [0.0] * (3 - D)))
        g = None if range_ is None else (C.c_double * 3)(*([float(x) for x in range_] + [0.0] * (3 - D)))
        out = np.empty(self._ncell, dtype=np.int8)
        _abi.check(self._ctx, _abi.lib().mplx_update_potential_map(self._ctx, p, r, g, float(power), out.ctypes.data))
        self.has_potential = True
        return out

    def setSearchRegion(self, path, search_radius, dense=False):
        """MapPlanner::setSearchRegion: installs the tunnel around `path` ([n][D]) and returns it, one byte
        per cell.  `dense` has the reference's (inverted) meaning: False = ray-trace between the points."""
        D = len(self.map_dim)
        pts = np.ascontiguousarray(path, dtype=np.float64).reshape(-1, D)
        sr = (C.c_double * 3)(*([float(x) for x in search_radius] + [0.0] * (3 - D)))
        out = np.empty(self._ncell, dtype=np.uint8)
        _abi.check(self._ctx, _abi.lib().mplx_set_search_region_path(self._ctx, pts.ctypes.data, pts.shape[0],
                                                                      int(bool(dense)), sr, out.ctypes.data))
        return out

    # ---- MapUtil's own map operations on the device map (map_util.h:136-296, include/mplx_map_util.h); the potential
    #      map, if one is installed, is a separate copy and stays as it is
    def _map_out(self, read_back):
        return np.empty(self._ncell, dtype=np.int8) if read_back else None

    def dilate(self, neighbors, read_back=True):
        """MapUtil::dilate: every cell an offset of `neighbors` ([n][D] ints) reaches from a cell occupied before the
        call becomes 100.  Returns the new int8 map (read_back=True) or None."""
        D = len(self.map_dim)
        off = np.ascontiguousarray(np.asarray(neighbors, dtype=np.int64).reshape(-1, D), dtype=np.int32)
        out = self._map_out(read_back)
        _abi.check(self._ctx, _abi.lib().mplx_map_dilate(self._ctx, off.ctypes.data, off.shape[0],
                                                         None if out is None else out.ctypes.data))
        return out

    def freeUnknown(self, read_back=True):
        """MapUtil::freeUnknown: unknown cells (-1) become free (0)."""
        out = self._map_out(read_back)
        _abi.check(self._ctx, _abi.lib().mplx_map_free(self._ctx, 1, None if out is None else out.ctypes.data))
        return out

    def freeAll(self, read_back=True):
        """MapUtil::freeAll: every cell becomes free (0)."""
        out = self._map_out(read_back)
        _abi.check(self._ctx, _abi.lib().mplx_map_free(self._ctx, 0, None if out is None else out.ctypes.data))
        return out

    def _cloud(self, kind):
        L = _abi.lib()
        n = C.c_int64(0)
        _abi.check(self._ctx, L.mplx_map_cloud(self._ctx, kind, None, 0, C.byref(n)))
        pts = np.empty((n.value, len(self.map_dim)), dtype=np.float64)
        if n.value:
            _abi.check(self._ctx, L.mplx_map_cloud(self._ctx, kind, pts.ctypes.data, n.value, C.byref(n)))
        return pts

    def getCloud(self):
        """MapUtil::getCloud: centres of the occupied cells, (n, D) float64, x outermost as the reference loops."""
        return self._cloud(_abi.CELL_OCCUPIED)

    def getFreeCloud(self):
        return self._cloud(_abi.CELL_FREE)

    def getUnknownCloud(self):
        return self._cloud(_abi.CELL_UNKNOWN)

    def _flush(self):
        if self._dirty:
            _abi.check(self._ctx, _abi.lib().mplx_set_params(self._ctx, C.byref(self._p)))
            self._dirty = False

    # ---- get_succ, exactly the reference's contract (env_map.h:147-172)
    def get_succ(self, curr):
        """Returns (succ, succ_cost, action_idx): successors in ascending control
        index; blocked ones are included with cost = +inf."""
        self.set_control(curr.control) if curr.control != self._p.control else None
        self._flush()
        F, nU = self.n_fields, self.nU
        node = np.ascontiguousarray(curr.to_row(), dtype=np.float64)
        succ = np.empty((nU, F), dtype=np.float64)
        cost = np.empty(nU, dtype=np.float64)
        act = np.empty(nU, dtype=np.int32)
        n = C.c_int32()
        _abi.check(self._ctx, _abi.lib().mplx_get_succ(self._ctx, node.ctypes.data, succ.ctypes.data,
                                                        cost.ctypes.data, act.ctypes.data, C.byref(n)))
        m = n.value
        return ([Waypoint.from_row(self.dim, curr.control, succ[i]) for i in range(m)],
                cost[:m].tolist(), act[:m].tolist())

    # ---- batched forms
    def expand(self, nodes, want_state=True, want_iters=True):
        """Dense expansion of a host frontier [4D+2][N]; returns host arrays."""
        self._flush()
        nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        if nodes.ndim != 2 or nodes.shape[0] != self.n_fields:
            raise ValueError("nodes must be [%d][N]" % self.n_fields)
        n = nodes.shape[1]
        ns = n * self.nU
        out = {"status": np.empty(ns, np.uint8), "cost": np.empty(ns, np.float64),
               "hash": np.empty(ns, np.uint64)}
        s = _abi.Succ()
        s.status, s.cost, s.hash = out["status"].ctypes.data, out["cost"].ctypes.data, out["hash"].ctypes.data
        if want_state:
            out["state"] = np.empty((self.n_fields, ns), np.float64)
            s.state, s.state_stride = out["state"].ctypes.data, ns
        if want_iters:
            out["iters"] = np.empty(ns, np.int32)
            s.iters = out["iters"].ctypes.data
        _abi.check(self._ctx, _abi.lib().mplx_expand(self._ctx, nodes.ctypes.data, n, n, C.byref(s)))
        return out

    def expand_lists(self, nodes, want_state=True, want_iters=True, stride=None, out=None):
        """Per-node successor lists of a host frontier [4D+2][N] (mplx_expand_lists).
        `stride` = entries reserved per node (default nU; out["stride"] reports it).
        `out` = the dict a previous call with the same shapes returned: its arrays are reused (a C caller
        keeps its buffers too; fresh arrays cost one page fault per 4 KiB written)."""
        self._flush()
        nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        if nodes.ndim != 2 or nodes.shape[0] != self.n_fields:
            raise ValueError("nodes must be [%d][N]" % self.n_fields)
        n = nodes.shape[1]
        stride = self.nU if stride is None else int(stride)
        ns = n * stride
        reuse = out is not None
        if reuse:
            if out["stride"] != stride or out["count"].shape != (n,) or (want_state and "state" not in out) or (
                    want_iters and "iters" not in out):
                raise ValueError("out does not match this call")
        else:
            out = {"stride": stride, "count": np.zeros(n, np.int32), "action": np.zeros(ns, np.int32),
                   "cost": np.zeros(ns, np.float64), "hash": np.zeros(ns, np.uint64)}
        s = _abi.SuccLists()
        s.node_stride = stride
        s.count, s.action = out["count"].ctypes.data, out["action"].ctypes.data
        s.cost, s.hash = out["cost"].ctypes.data, out["hash"].ctypes.data
        if want_state:
            if not reuse:
                out["state"] = np.zeros((self.n_fields, ns), np.float64)
            s.state, s.state_stride = out["state"].ctypes.data, ns
        if want_iters:
            if not reuse:
                out["iters"] = np.zeros(ns, np.int32)
            s.iters = out["iters"].ctypes.data
        _abi.check(self._ctx, _abi.lib().mplx_expand_lists(self._ctx, nodes.ctypes.data, n, n, C.byref(s)))
        return out

    def alloc_lists(self, n_nodes, want_state=True, want_iters=False, want_hash=True, stride=None, alloc=None,
                    state_pad=None, want_heur=False, want_flags=False):
        return Lists(self, n_nodes, self.nU, want_state, want_iters, want_hash, stride, alloc, state_pad, want_heur, want_flags)

    def set_goal(self, goal_row, w=None, v_max=None, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0, tol_yaw=-1.0, goal_control=0):
        """env_base::set_goal for the device (mplx_set_goal): the goal the `heur` / `flags` rows of the lists refer to.
        goal_row=None clears it."""
        self._flush()
        if goal_row is None:
            _abi.check(self._ctx, _abi.lib().mplx_set_goal(self._ctx, None))
            return
        goal = np.ascontiguousarray(goal_row, dtype=np.float64)
        g = _abi.GoalSpec()
        g.goal, g.control, g.goal_control = goal.ctypes.data, int(self._p.control), int(goal_control)
        g.w = float(self._p.w if w is None else w)
        g.v_max = float(self._p.v_max if v_max is None else v_max)
        g.tol_pos, g.tol_vel, g.tol_acc, g.tol_yaw = float(tol_pos), float(tol_vel), float(tol_acc), float(tol_yaw)
        _abi.check(self._ctx, _abi.lib().mplx_set_goal(self._ctx, C.byref(g)))

    def alloc_packed(self, n_nodes, capacity=None, want_state=True, want_hash=True, alloc=None):
        """Packed lists for n_nodes nodes; the default capacity n_nodes * nU always suffices."""
        return PackedLists(self, n_nodes, n_nodes * self.nU if capacity is None else capacity, want_state, want_hash, alloc)

    def pack_lists(self, lists, packed, n_nodes=None, want_total=False):
        """mplx_pack_lists_device: asynchronous unless want_total (then returns the number of packed entries)."""
        n = lists.n_nodes if n_nodes is None else int(n_nodes)
        s, p = lists.c_struct(), packed.c_struct()
        total = C.c_int64(-1)
        _abi.check(self._ctx, _abi.lib().mplx_pack_lists_device(self._ctx, C.byref(s), n, C.byref(p),
                                                                 C.byref(total) if want_total else None))
        return total.value if want_total else None

    # ---- RCCL communicator of the context (mplx_comm_*)
    @staticmethod
    def comm_unique_id():
        buf = (C.c_uint8 * _abi.COMM_ID_BYTES)()
        rc = _abi.lib().mplx_comm_unique_id(buf)
        if rc != _abi.OK:
            msg = _abi.lib().mplx_last_error(None)
            raise _abi.MplxError(rc, msg.decode() if msg else "?")
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * _abi.COMM_ID_BYTES).from_buffer_copy(unique_id)
        _abi.check(self._ctx, _abi.lib().mplx_comm_init(self._ctx, buf, int(rank), int(world)))

    def comm_destroy(self):
        _abi.check(self._ctx, _abi.lib().mplx_comm_destroy(self._ctx))

    def comm_broadcast_map(self, root=0):
        _abi.check(self._ctx, _abi.lib().mplx_comm_broadcast_map(self._ctx, int(root)))

    def comm_allgather_lists(self, local, n_local, gathered):
        """mplx_comm_allgather_lists; returns (node_offs, entry_offs) per rank, each [world + 1]."""
        a, b = local.c_struct(), gathered.c_struct()
        no = np.zeros(1025, np.int64)
        eo = np.zeros(1025, np.int64)
        _abi.check(self._ctx, _abi.lib().mplx_comm_allgather_lists(self._ctx, C.byref(a), int(n_local), C.byref(b),
                                                                    no.ctypes.data, eo.ctypes.data))
        return no, eo

    def expand_lists_resident(self, frontier, lists, n_nodes=None):
        """Asynchronous launch on HBM-resident buffers: mplx_expand_lists_device_z for lists that carry the mask of
        their all-zero state rows (`zero_rows`, env.Lists), mplx_expand_lists_device for any other object."""
        self._flush()
        n = frontier.n_nodes if n_nodes is None else int(n_nodes)
        s = lists.c_struct()
        if hasattr(lists, "zero_rows"):
            m = C.c_uint32(int(lists.zero_rows))
            lists.zero_rows = 0  # (a call that fails on the way promises nothing)
            _abi.check(self._ctx, _abi.lib().mplx_expand_lists_device_z(self._ctx, frontier.ptr, n, frontier.n_nodes,
                                                                        C.byref(s), C.byref(m)))
            lists.zero_rows = int(m.value)
            return
        _abi.check(self._ctx, _abi.lib().mplx_expand_lists_device(self._ctx, frontier.ptr, n, frontier.n_nodes,
                                                                  C.byref(s)))

    def post_lists(self, lists, goal_row, w=None, v_max=None, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0, tol_yaw=-1.0,
                   n_nodes=None, want_canon=True):
        """Heuristic, goal-tolerance flags and node identity of HBM-resident lists
        (mplx_post_lists_device).  Returns host arrays indexed like the lists."""
        self._flush()
        n = lists.n_nodes if n_nodes is None else int(n_nodes)
        goal = np.ascontiguousarray(goal_row, dtype=np.float64)
        g = _abi.GoalSpec()
        g.goal, g.control = goal.ctypes.data, int(self._p.control)
        g.w = float(self._p.w if w is None else w)
        g.v_max = float(self._p.v_max if v_max is None else v_max)
        g.tol_pos, g.tol_vel, g.tol_acc, g.tol_yaw = float(tol_pos), float(tol_vel), float(tol_acc), float(tol_yaw)
        ns = lists.n_slots
        heur = DeviceArray(self, max(ns, 1) * 8)
        flags = DeviceArray(self, max(ns, 1))
        canon = DeviceArray(self, max(ns, 1) * 4) if want_canon else None
        _abi.check(self._ctx, _abi.lib().mplx_memset(self._ctx, flags.ptr, 0, max(ns, 1)))
        o = _abi.Post()
        o.heur, o.flags, o.canon = heur.ptr, flags.ptr, canon.ptr if canon else None
        s = lists.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_post_lists_device(self._ctx, C.byref(s), n, C.byref(g), C.byref(o)))
        self.synchronize()
        out = {"heur": heur.download(np.float64, (ns,)), "flags": flags.download(np.uint8, (ns,))}
        if canon:
            out["canon"] = canon.download(np.int32, (ns,))
            canon.free()
        heur.free()
        flags.free()
        return out

    def post_packed(self, packed, n_nodes, goal_row, w=None, v_max=None, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0,
                    tol_yaw=-1.0, want_canon=True, alloc=None, download=True):
        """mplx_post_packed_device: heuristic, goal flags and node identity of PACKED lists (e.g. the gathered lists
        of all ranks).  `packed`: an env.PackedLists or a ready _abi.PackedLists struct (device pointers).  Returns
        host arrays (download=True) or the device buffers {"heur", "flags", "canon"} (asynchronous)."""
        self._flush()
        ps = packed.c_struct() if hasattr(packed, "c_struct") else packed
        cap = int(ps.capacity)
        goal = np.ascontiguousarray(goal_row, dtype=np.float64)
        g = _abi.GoalSpec()
        g.goal, g.control = goal.ctypes.data, int(self._p.control)
        g.w = float(self._p.w if w is None else w)
        g.v_max = float(self._p.v_max if v_max is None else v_max)
        g.tol_pos, g.tol_vel, g.tol_acc, g.tol_yaw = float(tol_pos), float(tol_vel), float(tol_acc), float(tol_yaw)
        heur = _alloc(self, cap * 8, alloc)
        flags = _alloc(self, cap, alloc)
        canon = _alloc(self, cap * 4, alloc) if want_canon else None
        _abi.check(self._ctx, _abi.lib().mplx_memset(self._ctx, flags.ptr, 0, cap))
        o = _abi.Post()
        o.heur, o.flags, o.canon = heur.ptr, flags.ptr, canon.ptr if canon else None
        _abi.check(self._ctx, _abi.lib().mplx_post_packed_device(self._ctx, C.byref(ps), int(n_nodes), C.byref(g), C.byref(o)))
        if not download:
            return {"heur": heur, "flags": flags, "canon": canon}
        self.synchronize()
        total = int(DeviceArrayView(self, ps.offs).download_i64(int(n_nodes)))
        out = {"heur": heur.download(np.float64, (total,)), "flags": flags.download(np.uint8, (total,)), "total": total}
        if canon:
            out["canon"] = canon.download(np.int32, (total,))
            canon.free()
        heur.free()
        flags.free()
        return out

    def check_edges(self, parents, actions, cell_cap=0):
        """Batched env_map::is_free(Primitive) + calculate_intrinsic_cost (+ the linked cells of
        MapPlanner::getLinkedNodes when cell_cap > 0) for edges (parent column, action id)."""
        self._flush()
        parents = np.ascontiguousarray(parents, dtype=np.float64)
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        n = actions.size
        if parents.ndim != 2 or parents.shape != (self.n_fields, n):
            raise ValueError("parents must be [%d][%d]" % (self.n_fields, n))
        out = {"free": np.zeros(n, np.uint8), "cost": np.zeros(n, np.float64)}
        o = _abi.EdgesOut()
        o.free_flag, o.cost = out["free"].ctypes.data, out["cost"].ctypes.data
        if cell_cap > 0:
            out["cells"] = np.zeros((n, int(cell_cap)), np.int32)
            out["cell_count"] = np.zeros(n, np.int32)
            o.cells, o.cell_count, o.cell_cap = out["cells"].ctypes.data, out["cell_count"].ctypes.data, int(cell_cap)
        _abi.check(self._ctx, _abi.lib().mplx_check_edges(self._ctx, parents.ctypes.data, actions.ctypes.data, n, n,
                                                           C.byref(o)))
        return out

    def upload_frontier(self, nodes):
        nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        if nodes.ndim != 2 or nodes.shape[0] != self.n_fields:
            raise ValueError("nodes must be [%d][N]" % self.n_fields)
        buf = DeviceArray(self, max(nodes.nbytes, 8))
        buf.upload(nodes)
        buf.n_nodes = nodes.shape[1]
        return buf

    def alloc_slots(self, n_nodes, want_state=True, want_iters=False):
        return Slots(self, n_nodes, self.nU, want_state, want_iters)

    def expand_resident(self, frontier, slots, n_nodes=None, node_offset=0):
        """Asynchronous launch on HBM-resident buffers (mplx_expand_device)."""
        self._flush()
        n = frontier.n_nodes if n_nodes is None else int(n_nodes)
        s = slots.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_expand_device(
            self._ctx, frontier.ptr + 8 * int(node_offset), n, frontier.n_nodes, C.byref(s)))

    # ---- batched rollouts (include/mplx_rollout.h): cost and validity of action sequences on the device map
    def rollout(self, starts, actions, want_end=True, want_goal_rows=False):
        """K action sequences from their start states, one pair per step with the primitive, the limits and the cost
        of get_succ, on the map the device holds now (mplx_rollout; synchronous).
        starts: [4D+2][K], or one state ([4D+2] / [4D+2][1]) every rollout starts from; actions: [H][K] indices into
        the control table, -1 ends a sequence early.  Returns numpy arrays: status (SLOT_* of the step that stopped the
        rollout, SLOT_FINITE when it is complete, ROLLOUT_BAD_ACTION), steps, cost (+inf unless complete), prefix_cost;
        want_end: end_state [4D+2][K], end_hash; want_goal_rows (needs set_goal): end_heur, end_flags."""
        self._flush()
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        if actions.ndim != 2 or actions.shape[0] < 1:
            raise ValueError("actions must be [H][K] with H >= 1")
        H, K = actions.shape
        starts = np.ascontiguousarray(starts, dtype=np.float64)
        if starts.ndim == 1:
            starts = starts.reshape(-1, 1)
        if starts.shape[0] != self.n_fields or starts.shape[1] not in (1, K):
            raise ValueError("starts must be [%d][%d] or one state" % (self.n_fields, K))
        out, o = Rollouts.host(self, K, want_end, want_goal_rows)
        _abi.check(self._ctx, _abi.lib().mplx_rollout(self._ctx, starts.ctypes.data, starts.shape[1], starts.shape[1],
                                                       actions.ctypes.data, K, H, K, C.byref(o)))
        return out

    def alloc_rollouts(self, n_rollouts, want_end=True, want_goal_rows=False):
        return Rollouts(self, n_rollouts, want_end, want_goal_rows)

    def rollout_resident(self, starts, actions, out, horizon, n_rollouts=None, n_starts=None, start_stride=None,
                         action_stride=None):
        """Asynchronous launch on HBM-resident buffers (mplx_rollout_device).  starts: float64 [4D+2][start_stride],
        actions: int32 [horizon][action_stride], each a DeviceArray or anything with .ptr / data_ptr() -- a torch tensor
        on the device is read in place, without a copy; out: env.Rollouts (alloc_rollouts).  n_starts: n_rollouts or 1
        (default: start_stride); the strides default to n_rollouts.  Rollouts that met a heading-limit decision
        inside the band of the yaw pinning carry ROLLOUT_HEADING_BAND in their status (rollout() resolves them).
        The launch runs on the CONTEXT's stream: a caller that filled the inputs on another stream (torch's) makes
        that stream finish first (torch.cuda.synchronize() or an event), and calls synchronize() before it reads
        `out` or overwrites the inputs."""
        self._flush()
        n = out.n if n_rollouts is None else int(n_rollouts)
        if n > out.n:
            raise ValueError("out holds %d rollouts, %d asked for" % (out.n, n))
        sstride = n if start_stride is None else int(start_stride)
        if n_starts is None:
            n_starts = n if start_stride is None else sstride
        astride = n if action_stride is None else int(action_stride)
        o = out.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_rollout_device(self._ctx, _device_ptr(starts), int(n_starts), sstride,
                                                              _device_ptr(actions), n, int(horizon), astride, C.byref(o)))

    # ---- MapUtil::rayTrace and the ray trace of is_goal on the device map (include/mplx_ray.h)
    def ray_trace(self, p1, p2, cell_cap=0, lanes=0, cells=None):
        """MapUtil::rayTrace for n point pairs on the int8 map the device holds now (mplx_ray_trace; synchronous).
        p1: [D][n] field-major like node rows (or one point [D]); p2: [D][n], or one point [D] every ray ends at.
        Returns numpy arrays: status (RAY_LEFT_MAP | RAY_HIT | RAY_BAD | RAY_TRUNCATED bits), n_cells (the length of
        the reference's list), first_hit (getIndex of the first occupied cell of the list, -1 without one) and, with
        cell_cap > 0, cells [n][cell_cap]: getIndex of the first cell_cap emitted cells in order, the entries past
        min(n_cells, cell_cap) untouched (`cells`: the array to write into, default zeros).  lanes: 0 (automatic) or
        4 / 16 / 64 lanes of a wavefront per ray; the results do not depend on it."""
        D = self.dim
        p1 = np.ascontiguousarray(p1, dtype=np.float64)
        if p1.ndim == 1:
            p1 = p1.reshape(D, 1)
        if p1.ndim != 2 or p1.shape[0] != D:
            raise ValueError("p1 must be [%d][n]" % D)
        n = p1.shape[1]
        p2 = np.ascontiguousarray(p2, dtype=np.float64)
        if p2.shape == (D,):
            p2_stride = 0
        elif p2.shape == (D, n):
            p2_stride = n
        else:
            raise ValueError("p2 must be [%d][%d] or one point" % (D, n))
        out, o = Rays.host(self, n, cell_cap)
        if cell_cap > 0 and cells is not None:  # the caller's array instead of zeros
            if cells.shape != (n, int(cell_cap)) or cells.dtype != np.int32 or not cells.flags.c_contiguous:
                raise ValueError("cells must be a contiguous int32 [%d][%d]" % (n, cell_cap))
            out["cells"], o.cells = cells, cells.ctypes.data
        _abi.check(self._ctx, _abi.lib().mplx_ray_trace(self._ctx, p1.ctypes.data, p2.ctypes.data, n, n, p2_stride,
                                                         int(lanes), C.byref(o)))
        return out

    def alloc_rays(self, n, cell_cap=0, want_counts=True):
        return Rays(self, n, cell_cap, want_counts)

    def ray_trace_resident(self, p1, p2, out, n=None, stride=None, p2_stride=None, lanes=0):
        """Asynchronous launch on HBM-resident buffers (mplx_ray_trace_device).  p1, p2: float64 [D][stride] /
        [D][p2_stride], each a DeviceArray or anything with .ptr / data_ptr(); p2_stride=0: p2 is one point (D doubles).
        out: env.Rays (alloc_rays).  The strides default to n.  Runs on the context's stream: synchronize() before
        reading `out`."""
        n = out.n if n is None else int(n)
        if n > out.n:
            raise ValueError("out holds %d rays, %d asked for" % (out.n, n))
        stride = n if stride is None else int(stride)
        p2_stride = n if p2_stride is None else int(p2_stride)
        o = out.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_ray_trace_device(self._ctx, _device_ptr(p1), _device_ptr(p2), n, stride,
                                                                p2_stride, int(lanes), C.byref(o)))

    def goal_sight(self, lists, flags=None, goal_row=None, tol_pos=0.5, n_nodes=None):
        """The ray trace of env_map::is_goal (env_map.h:38-43) on HBM-resident lists (mplx_goal_sight_device;
        asynchronous): every emitted successor whose flags byte has bit 0 (inside the goal tolerances) and whose ray
        to the goal position meets an occupied cell gets FLAG_GOAL_BLOCKED ORed in; afterwards (flags & 9) == 1 is
        the reference's is_goal.  flags: the device row to work on (default lists.flags, the row the expansion
        launch wrote).  goal_row: the goal waypoint (with tol_pos) instead of the one of set_goal."""
        self._flush()
        n = lists.n_nodes if n_nodes is None else int(n_nodes)
        s = lists.c_struct()
        fl = lists.flags if flags is None else flags
        g = None
        if goal_row is not None:
            goal = np.ascontiguousarray(goal_row, dtype=np.float64)
            g = _abi.GoalSpec()
            g.goal, g.control, g.tol_pos = goal.ctypes.data, int(self._p.control), float(tol_pos)
            g.w, g.v_max = float(self._p.w), float(self._p.v_max)
            g.tol_vel = g.tol_acc = g.tol_yaw = -1.0
        _abi.check(self._ctx, _abi.lib().mplx_goal_sight_device(self._ctx, C.byref(s), n, None if g is None else C.byref(g),
                                                                 None if fl is None else _device_ptr(fl)))

    # ---- Trajectory<Dim> on the device (include/mplx_traj.h): info, samples, traverse_trajectory
    def _traj_host_set(self, starts, actions):
        actions = np.ascontiguousarray(actions, dtype=np.int32)
        if actions.ndim == 1:
            actions = actions.reshape(-1, 1)
        if actions.ndim != 2 or actions.shape[0] < 1:
            raise ValueError("actions must be [H][K] with H >= 1")
        H, K = actions.shape
        starts = np.ascontiguousarray(starts, dtype=np.float64)
        if starts.ndim == 1:
            starts = starts.reshape(-1, 1)
        if starts.shape[0] != self.n_fields or starts.shape[1] not in (1, K):
            raise ValueError("starts must be [%d][%d] or one state" % (self.n_fields, K))
        s = _abi.TrajSet()
        s.starts, s.n_starts, s.start_stride = starts.ctypes.data, starts.shape[1], starts.shape[1]
        s.actions, s.n_traj, s.horizon, s.action_stride = actions.ctypes.data, K, H, K
        return s, (starts, actions), K, H

    def _traj_device_set(self, starts, actions, horizon, n_traj, n_starts, start_stride, action_stride):
        n = int(n_traj)
        sstride = n if start_stride is None else int(start_stride)
        if n_starts is None:
            n_starts = n if start_stride is None else sstride
        s = _abi.TrajSet()
        s.starts, s.n_starts, s.start_stride = _device_ptr(starts), int(n_starts), sstride
        s.actions, s.n_traj, s.horizon = _device_ptr(actions), n, int(horizon)
        s.action_stride = n if action_stride is None else int(action_stride)
        return s

    def traj_info(self, starts, actions, want_states=False):
        """Per trajectory (start state + action sequence, as rollout() takes them; -1 ends a sequence): status (TRAJ_EMPTY
        | TRAJ_BAD_ACTION), n_segs, total_time, effort [5][K] = J(VEL), J(ACC), J(JRK), J(SNP), Jyaw of
        Trajectory<Dim>; want_states: seg_state [4D+2][H+1][K], the chain states (entries past n_segs: zero).
        No validity check of any kind is made (mplx_traj_info; synchronous)."""
        self._flush()
        s, keep, K, H = self._traj_host_set(starts, actions)
        out, o = TrajInfo.host(self, K, H, want_states)
        _abi.check(self._ctx, _abi.lib().mplx_traj_info(self._ctx, C.byref(s), C.byref(o)))
        return out

    def _traj_times(self, N, times, form, K):
        t = _abi.TrajTimes()
        t.form = int(form)
        if (N is None) == (times is None):
            raise ValueError("give N (uniform samples) or times, not both")
        if N is not None:
            t.n_uniform = int(N)
            return t, None, int(N) + 1
        times = np.ascontiguousarray(times, dtype=np.float64)
        if times.ndim == 1:
            t.n_times, t.time_stride = times.shape[0], 0
        elif times.ndim == 2 and times.shape[0] == K:
            t.n_times, t.time_stride = times.shape[1], times.shape[1]
        else:
            raise ValueError("times must be [Q] (shared) or [K][Q] (one column per trajectory)")
        t.times = times.ctypes.data
        return t, times, int(t.n_times)

    def traj_sample(self, starts, actions, N=None, times=None, form=TRAJ_COMMAND, out=None):
        """Samples of K trajectories (mplx_traj_sample; synchronous).  N: Trajectory::sample(N), the N + 1 uniform times
        i * (T / N); or times: [Q] shared or [K][Q].  form TRAJ_COMMAND: rows pos, vel, acc, jrk, yaw, yaw_dot, t of
        Trajectory::evaluate(t, Command&); TRAJ_WAYPOINT: the first 4D+1 rows of evaluate(t) -> Waypoint, the last two
        untouched.  Returns samples [4D+3][K][count] (`out`: a C-contiguous float64 [4D+3][>= K][>= count] to write
        into instead of zeros; entries the call does not own keep their values) and status [K]."""
        self._flush()
        s, keep, K, H = self._traj_host_set(starts, actions)
        t, tkeep, count = self._traj_times(N, times, form, K)
        rows = 4 * self.dim + 3
        if out is None:
            out = np.zeros((rows, K, max(count, 0)), np.float64)
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.ndim != 3 or out.shape[0] != rows:
            raise ValueError("out must be a C-contiguous float64 [%d][K'][count']" % rows)
        status = np.zeros(K, np.uint8)
        o = _abi.TrajSampleOut()
        o.out, o.row_stride, o.sample_stride, o.status = out.ctypes.data, out.shape[1] * out.shape[2], out.shape[2], status.ctypes.data
        if out.shape[1] < K:
            raise ValueError("out holds %d trajectories, %d asked for" % (out.shape[1], K))
        _abi.check(self._ctx, _abi.lib().mplx_traj_sample(self._ctx, C.byref(s), C.byref(t), C.byref(o)))
        return {"samples": out, "status": status}

    def traj_traverse(self, starts, actions, lanes=0):
        """env_map::traverse_trajectory of K trajectories on the maps the device holds now (mplx_traj_traverse;
        synchronous): cost (0.0, a finite sum of potential terms, or +inf), n_samples, n_cells (samples not skipped),
        stop_sample (the sample that made the cost +inf, -1), status (TRAJ_EMPTY | TRAJ_BAD_ACTION | TRAJ_BAD).
        lanes: 0 (automatic) or 4 / 16 / 64 lanes of a wavefront per trajectory; the results do not depend on it."""
        self._flush()
        s, keep, K, H = self._traj_host_set(starts, actions)
        out, o = TrajTraverse.host(self, K)
        _abi.check(self._ctx, _abi.lib().mplx_traj_traverse(self._ctx, C.byref(s), int(lanes), C.byref(o)))
        return out

    def alloc_traj_info(self, n, horizon, want_states=False):
        return TrajInfo(self, n, horizon, want_states)

    def alloc_traj_samples(self, n, count, n_stride=None, sample_stride=None):
        return TrajSamples(self, n, count, n_stride, sample_stride)

    def alloc_traj_traverse(self, n):
        return TrajTraverse(self, n)

    def traj_info_resident(self, starts, actions, out, horizon, n_traj=None, n_starts=None, start_stride=None,
                           action_stride=None):
        """Asynchronous on HBM-resident buffers (mplx_traj_info_device); starts / actions as rollout_resident takes
        them (DeviceArray or anything with .ptr / data_ptr()), out: env.TrajInfo.  synchronize() before reading."""
        self._flush()
        s = self._traj_device_set(starts, actions, horizon, out.n if n_traj is None else n_traj, n_starts, start_stride,
                                  action_stride)
        o = out.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_traj_info_device(self._ctx, C.byref(s), C.byref(o)))

    def traj_sample_resident(self, starts, actions, out, horizon, N=None, times=None, n_times=None, time_stride=0,
                             form=TRAJ_COMMAND, n_traj=None, n_starts=None, start_stride=None, action_stride=None):
        """Asynchronous (mplx_traj_sample_device).  N, or times: a device buffer of n_times values (time_stride 0:
        shared; >= n_times: trajectory k reads times[k * time_stride + i]).  out: env.TrajSamples."""
        self._flush()
        s = self._traj_device_set(starts, actions, horizon, out.n if n_traj is None else n_traj, n_starts, start_stride,
                                  action_stride)
        t = _abi.TrajTimes()
        t.form = int(form)
        if N is not None:
            t.n_uniform = int(N)
        else:
            t.times, t.n_times, t.time_stride = _device_ptr(times), int(n_times), int(time_stride)
        o = out.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_traj_sample_device(self._ctx, C.byref(s), C.byref(t), C.byref(o)))

    def traj_traverse_resident(self, starts, actions, out, horizon, lanes=0, n_traj=None, n_starts=None, start_stride=None,
                               action_stride=None):
        """Asynchronous (mplx_traj_traverse_device); out: env.TrajTraverse."""
        self._flush()
        s = self._traj_device_set(starts, actions, horizon, out.n if n_traj is None else n_traj, n_starts, start_stride,
                                  action_stride)
        o = out.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_traj_traverse_device(self._ctx, C.byref(s), int(lanes), C.byref(o)))

    # ---- conflicts between K action chains on a common clock (include/mplx_conflict.h); no map is needed
    def alloc_conflicts(self, n, want_pairs=False):
        return Conflicts(self, n, want_pairs)

    def traj_conflicts(self, starts, actions, step, n_steps=None, t0=None, radius=None, group=None, rank=None, park=True,
                       want_pairs=False, chunk_steps=0):
        """PolyTrajSet.conflicts for K action chains (starts / actions as traj_sample takes them; mplx_traj_conflicts;
        synchronous): positions are those of traj_sample at i * step - t0[k]; an EMPTY or BAD_ACTION chain is excluded.
        Returns a ConflictResult."""
        self._flush()
        s, keep, K, H = self._traj_host_set(starts, actions)
        if n_steps is None:
            inf = self.traj_info(starts, actions)
            n_steps = _conflict_steps(float(step), t0, inf["total_time"], inf["status"] == 0)
        i, ikeep = _conflict_in(K, step, n_steps, t0, radius, group, rank, park, chunk_steps, False)
        rows, o = _conflict_host_out(K, want_pairs)
        _abi.check(self._ctx, _abi.lib().mplx_traj_conflicts(self._ctx, C.byref(s), C.byref(i), C.byref(o)))
        return ConflictResult(step, rows["first_step"], rows["first_partner"], rows["min_d2"], rows["status"], rows.get("pair_first"))

    def traj_conflicts_resident(self, starts, actions, out, horizon, step, n_steps, t0=None, radius=None, group=None, rank=None,
                                park=True, chunk_steps=0, n_traj=None, n_starts=None, start_stride=None, action_stride=None):
        """Asynchronous (mplx_traj_conflicts_device); starts / actions as traj_sample_resident takes them, out:
        alloc_conflicts(n, want_pairs); t0 / radius / group / rank: device buffers of [K] (radius may be a scalar)."""
        self._flush()
        n = out.n if n_traj is None else n_traj
        s = self._traj_device_set(starts, actions, horizon, n, n_starts, start_stride, action_stride)
        i, keep = _conflict_in(int(n), step, n_steps, t0, radius, group, rank, park, chunk_steps, True)
        o = out.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_traj_conflicts_device(self._ctx, C.byref(s), C.byref(i), C.byref(o)))

    # ---- the trajectory solver (include/mplx_solve.h): TrajSolver / PolySolver::solve for K problems in one launch
    def alloc_poly(self, k_cap, w_max):
        return PolyTrajSet(self, k_cap, w_max)

    def alloc_solve_out(self, n, w_max, control=None):
        return SolveOut(self, n, w_max, _solve_order(self._p.control if control is None else control))

    def solve_traj(self, waypoints, n_wp=None, dts=None, v=1.0, control=None, wp_flags=None, yaw_control=VEL):
        """Minimum-velocity / acceleration / jerk polynomials through K waypoint lists (mplx_solve; synchronous).
        waypoints: state rows [4D+2][w_max][K] (the seg_state of traj_info(want_states=True)), or positions [D][w_max][K]
        (every other field zero); n_wp [K] or None (w_max each); dts [w_max - 1][K] or None: allocate_time with v, a
        scalar or [K]; control: of the two ends (default: the EnvMap's), VEL / ACC / JRK; wp_flags [w_max][K] USE_POS |
        USE_VEL | USE_ACC (TrajSolver::setWaypoints), or None: interior waypoints fix their position only
        (TrajSolver::setPath).  Returns a PolyTrajSet."""
        self._flush()
        control = int(self._p.control if control is None else control)
        so = _solve_order(control)
        wp = np.asarray(waypoints, dtype=np.float64)
        if wp.ndim == 2:
            wp = wp[:, :, None]
        if wp.ndim != 3 or wp.shape[0] not in (self.dim, self.n_fields):
            raise ValueError("waypoints must be [%d][w_max][K] or [%d][w_max][K]" % (self.n_fields, self.dim))
        if wp.shape[0] == self.dim:
            full = np.zeros((self.n_fields,) + wp.shape[1:])
            full[:self.dim] = wp
            wp = full
        wp = np.ascontiguousarray(wp)
        W, K = wp.shape[1], wp.shape[2]
        poly = PolyTrajSet(self, max(K, 1), max(W, 2))
        try:
            i = _abi.SolveIn()
            i.waypoints, i.n_prob, i.w_max, i.wp_stride = wp.ctypes.data, K, W, K
            keep = [wp]
            if n_wp is not None:
                n_wp = np.ascontiguousarray(np.broadcast_to(np.asarray(n_wp, dtype=np.int32), (K,)))
                i.n_wp = n_wp.ctypes.data
            if dts is not None:
                dts = np.ascontiguousarray(np.asarray(dts, dtype=np.float64).reshape(W - 1, K))
                i.dts, i.dt_stride = dts.ctypes.data, K
            if np.ndim(v) == 0:
                i.v = float(v)
            else:
                v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (K,)))
                i.v_arr = v.ctypes.data
            if wp_flags is not None:
                wp_flags = np.ascontiguousarray(np.asarray(wp_flags, dtype=np.uint8).reshape(W, K))
                i.wp_flags, i.flag_stride = wp_flags.ctypes.data, K
            i.control, i.yaw_control = control, int(yaw_control)
            host, o = SolveOut.host(self, K, W, so)
            _abi.check(self._ctx, _abi.lib().mplx_solve(poly._h, C.byref(i), C.byref(o)))
            poly.n, poly.so, poly.n_wmax, poly._host, poly.control = K, so, W, host, control
            poly._lambda = None  # a new solve or load clears the Lambda
            return poly
        except Exception:
            poly.free()
            raise

    def solve_traj_resident(self, poly, waypoints, n_prob, w_max, wp_stride=None, n_wp=None, dts=None, dt_stride=None, v=1.0,
                            v_arr=None, control=None, wp_flags=None, flag_stride=None, out=None, yaw_control=VEL):
        """Asynchronous on HBM-resident buffers (mplx_solve_device): waypoints / n_wp / dts / v_arr / wp_flags are
        DeviceArrays or anything with .ptr / data_ptr() (torch tensors); strides default to n_prob.  poly: alloc_poly;
        out: alloc_solve_out (then owned by poly: coefficients() / dts() / status download from it) or None."""
        self._flush()
        control = int(self._p.control if control is None else control)
        so = _solve_order(control)
        K = int(n_prob)
        i = _abi.SolveIn()
        i.waypoints, i.n_prob, i.w_max = _device_ptr(waypoints), K, int(w_max)
        i.wp_stride = K if wp_stride is None else int(wp_stride)
        if n_wp is not None:
            i.n_wp = _device_ptr(n_wp)
        if dts is not None:
            i.dts, i.dt_stride = _device_ptr(dts), K if dt_stride is None else int(dt_stride)
        i.v = float(v)
        if v_arr is not None:
            i.v_arr = _device_ptr(v_arr)
        if wp_flags is not None:
            i.wp_flags, i.flag_stride = _device_ptr(wp_flags), K if flag_stride is None else int(flag_stride)
        i.control, i.yaw_control = control, int(yaw_control)
        if out is not None and (out.n != K or out.w_max != int(w_max) or out.so != so):
            raise ValueError("out was allocated for another problem count, w_max or control")
        o = out.c_struct() if out is not None else _abi.SolveOut()
        _abi.check(self._ctx, _abi.lib().mplx_solve_device(poly._h, C.byref(i), C.byref(o)))
        if poly._out is not None and poly._out is not out:
            poly._out.free()
        poly.n, poly.so, poly.n_wmax, poly._host, poly._out, poly.control = K, so, int(w_max), None, out, control
        poly._lambda = None  # a new solve or load clears the Lambda
        return poly

    # ---- caller-given trajectories and two-point primitives (include/mplx_limits.h)
    def alloc_poly_limits(self, n):
        return PolyLimits(self, n)

    def alloc_lambda_rows(self, n, w_max, count=0):
        return LambdaRows(self, n, w_max, count)

    def load_traj(self, coeff, dts, n_segs=None, control=None):
        """K trajectories from their primitives (Primitive(cs, t, control) / Trajectory(prs); mplx_poly_load;
        synchronous).  coeff [S][D + 1][6][K]: c(0) .. c(5) of axis a of segment s at [s][a][:][k], axis D the yaw
        primitive (of which c(4), the rate, and c(5) are kept), or [S][D][6][K] (no yaw); dts [S][K]; n_segs [K] or None
        (S each); control: any of the eight flags (default: the EnvMap's).  Returns a PolyTrajSet: info / sample /
        traverse / limits as on a solved set."""
        self._flush()
        control = int(self._p.control if control is None else control)
        c = np.asarray(coeff, dtype=np.float64)
        if c.ndim == 3:
            c = c[..., None]
        if c.ndim != 4 or c.shape[1] not in (self.dim, self.dim + 1) or c.shape[2] != 6 or c.shape[0] < 1:
            raise ValueError("coeff must be [S >= 1][%d or %d][6][K]" % (self.dim, self.dim + 1))
        S, K = c.shape[0], c.shape[3]
        if c.shape[1] == self.dim:
            c = np.concatenate([c, np.zeros((S, 1, 6, K))], axis=1)
        c = np.ascontiguousarray(c)
        dts = np.ascontiguousarray(np.asarray(dts, dtype=np.float64).reshape(S, K))
        poly = PolyTrajSet(self, max(K, 1), S + 1)
        try:
            i = _abi.PolyLoadIn()
            i.n_prob, i.w_max, i.control = K, S + 1, control
            if n_segs is not None:
                n_segs = np.ascontiguousarray(np.broadcast_to(np.asarray(n_segs, dtype=np.int32), (K,)))
                i.n_segs = n_segs.ctypes.data
            i.dts, i.dt_stride, i.coeff, i.coeff_stride = dts.ctypes.data, K, c.ctypes.data, K
            host, o = LoadOut.host(self, K, S + 1)
            _abi.check(self._ctx, _abi.lib().mplx_poly_load(poly._h, C.byref(i), C.byref(o)))
            seg = np.arange(S)[:, None] < host["n_segs"][None, :]
            host["dts"] = np.where(seg, dts, 0.0)
            host["segments"] = np.where(seg[:, None, None, :], c, 0.0)
            poly.n, poly.so, poly.n_wmax, poly._host, poly.control = K, None, S + 1, host, control
            poly._lambda = None  # a new solve or load clears the Lambda
            return poly
        except Exception:
            poly.free()
            raise

    def alloc_load_out(self, n, w_max):
        return LoadOut(self, n, w_max)

    def load_traj_resident(self, poly, coeff, dts, n_prob, w_max, n_segs=None, control=None, coeff_stride=None, dt_stride=None,
                           out=None):
        """Asynchronous on HBM-resident buffers (mplx_poly_load_device): coeff / dts / n_segs are DeviceArrays or anything
        with .ptr / data_ptr(); strides default to n_prob.  poly: alloc_poly; out: alloc_load_out (then owned by poly, as
        the `out` of solve_traj_resident: status / n_segs / total_time / taus() download from it) or None: nothing of the
        set can be read on the host but what info / sample / traverse / limits return.  dts() and segments() are the
        caller's own arrays and are not kept."""
        self._flush()
        control = int(self._p.control if control is None else control)
        K = int(n_prob)
        i = _abi.PolyLoadIn()
        i.n_prob, i.w_max, i.control = K, int(w_max), control
        if n_segs is not None:
            i.n_segs = _device_ptr(n_segs)
        i.dts, i.dt_stride = _device_ptr(dts), K if dt_stride is None else int(dt_stride)
        i.coeff, i.coeff_stride = _device_ptr(coeff), K if coeff_stride is None else int(coeff_stride)
        if out is not None and (out.n != K or out.w_max != int(w_max)):
            raise ValueError("out was allocated for another problem count or w_max")
        o = out.c_struct() if out is not None else _abi.PolyLoadOut()
        _abi.check(self._ctx, _abi.lib().mplx_poly_load_device(poly._h, C.byref(i), C.byref(o)))
        if poly._out is not None and poly._out is not out:
            poly._out.free()
        poly.n, poly.so, poly.n_wmax, poly._host, poly._out, poly.control = K, None, int(w_max), None, out, control
        poly._lambda = None  # a new solve or load clears the Lambda
        return poly

    def shortcut_resident(self, states, n_query, w_max, n_wp=None, control=None, max_hop=None, stride=None, avoid=None, t0=None,
                          radius=None, ignore_group=None):
        """mplx_shortcut_device on chain states that are on the device already (the seg_state rows of
        traj_info_resident(want_states=True): field f of state w of query k at [(f w_max + w) stride + k]); n_wp [Q] on
        the device or None.  Everything is queued without a read-back; then counts, costs, statuses, the kept indices and
        the edge costs are read.  Returns a ShortcutResult.

        avoid: a search.Reservations: the timed shortcut (mplx_shortcut_timed_device, include/mplx_reserve_poly.h).  Chain
        k starts at t0[k] on the table's clock (its clock is t0 + the t row of its states), has radius[k] and ignores
        the reservations of ignore_group[k] (host values, [Q] or scalars; t0 default 0, radius required): they become the
        table's queries.  A hop is admitted only if it stays clear of the reservations inside the table's horizon; the
        chain's own edges stay admitted and ShortcutResult.chain_hit [Q] reports the first of them in conflict."""
        self._flush()
        control = int(self._p.control if control is None else control)
        so = _solve_order(control)
        Q, W = int(n_query), int(w_max)
        hop = W - 1 if max_hop is None else int(max_hop)
        if Q < 1 or W < 2 or hop < 1:
            raise ValueError("shortcut: needs Q >= 1, w_max >= 2 and max_hop >= 1")
        P = Q * (W - 1) * hop
        pairs, res = PolyTrajSet(self, P, 2), PolyTrajSet(self, Q, W)
        shapes = {"status": ((Q,), np.uint8), "n_keep": ((Q,), np.int32), "keep": ((W, Q), np.int32), "cost": ((Q,), np.float64),
                  "chain_cost": ((Q,), np.float64), "edge_cost": ((Q, W - 1, hop), np.float64)}
        if avoid is not None:
            if radius is None:
                raise ValueError("shortcut: avoid needs a radius")
            avoid.set_queries(np.broadcast_to(np.asarray(0.0 if t0 is None else t0, dtype=np.float64), (Q,)), radius, ignore_group)
            shapes["chain_hit"] = ((Q,), np.int64)
        elif t0 is not None or radius is not None or ignore_group is not None:
            raise ValueError("shortcut: t0 / radius / ignore_group go with avoid")
        bufs = {}
        try:
            pair_out = SolveOut(self, P, 2, so)
            pairs._out = pair_out
            i, o = _abi.ShortcutIn(), _abi.ShortcutOut()
            i.states, i.n_query, i.w_max, i.control, i.max_hop = _device_ptr(states), Q, W, control, hop
            i.stride = Q if stride is None else int(stride)
            if n_wp is not None:
                i.n_wp = _device_ptr(n_wp)
            for key, (shape, dt) in shapes.items():
                bufs[key] = DeviceArray(self, int(np.prod(shape)) * np.dtype(dt).itemsize)
                if key != "chain_hit":
                    setattr(o, key, bufs[key].ptr)
            o.keep_stride = Q
            po = pair_out.c_struct()
            o.pair_out = C.pointer(po)
            if avoid is None:
                _abi.check(self._ctx, _abi.lib().mplx_shortcut_device(pairs._h, res._h, C.byref(i), C.byref(o)))
            else:
                _abi.check(self._ctx, _abi.lib().mplx_shortcut_timed_device(pairs._h, res._h, C.byref(i), C.byref(o), avoid._res,
                                                                          bufs["chain_hit"].ptr))
            self.synchronize()
            rows = {key: bufs[key].download(dt, shape) for key, (shape, dt) in shapes.items()}
            pairs.n, pairs.so, pairs.n_wmax, pairs.control = P, so, 2, control
            res.n, res.so, res.n_wmax, res.control = Q, None, W, control
            info = res.info(want_states=True)
            S = info["n_segs"]
            taus = np.where(np.arange(W)[:, None] <= S[None, :], info["seg_state"][self.n_fields - 1], 0.0) * (S > 0)[None, :]
            res._host = {"status": info["status"], "n_segs": S, "total_time": info["total_time"], "taus": taus}
            return ShortcutResult(res, pairs, hop, rows)
        except Exception:
            pairs.free()
            res.free()
            raise
        finally:
            for b in bufs.values():
                b.free()

    def shortcut(self, states, n_wp=None, control=None, max_hop=None, avoid=None, t0=None, radius=None, ignore_group=None):
        """Shortcuts Q chains of states by two-point primitives (mplx_shortcut, include/mplx_limits.h):
        states [4D+2][w_max][Q] (the seg_state of traj_info(want_states=True)), n_wp [Q] or None (w_max each), control
        VEL / ACC / JRK (default: the EnvMap's), max_hop (default: w_max - 1).  Needs a map and v_max > 0.  Returns a
        ShortcutResult.  avoid / t0 / radius / ignore_group: the timed shortcut, as shortcut_resident takes them."""
        st = np.ascontiguousarray(np.asarray(states, dtype=np.float64))
        if st.ndim == 2:
            st = st[:, :, None]
        if st.ndim != 3 or st.shape[0] != self.n_fields:
            raise ValueError("states must be [%d][w_max][Q]" % self.n_fields)
        W, Q = st.shape[1], st.shape[2]
        d_st = DeviceArray(self, max(st.nbytes, 8))
        d_n = None
        try:
            d_st.upload(st)
            if n_wp is not None:
                n_wp = np.ascontiguousarray(np.broadcast_to(np.asarray(n_wp, dtype=np.int32), (Q,)))
                d_n = DeviceArray(self, n_wp.nbytes)
                d_n.upload(n_wp)
            return self.shortcut_resident(d_st, Q, W, n_wp=d_n, control=control, max_hop=max_hop, avoid=avoid, t0=t0, radius=radius,
                                          ignore_group=ignore_group)
        finally:
            d_st.free()
            if d_n is not None:
                d_n.free()

    def connect(self, p1_rows, p2_rows, T, control=None):
        """K two-point primitives Primitive(p1, p2, t) (primitive.h:54-83, 283-302): state rows [4D+2][K] of the two ends
        and durations T (a scalar or [K]) -> a PolyTrajSet of K one-segment trajectories, through solve_traj with every
        derivative up to the control's order fixed at both ends.  The coefficients equal the reference's up to rounding,
        not bit for bit: the reference forms A.inverse() * b with Eigen, this solver an elimination of its own."""
        a, b = (np.asarray(x, dtype=np.float64).reshape(self.n_fields, -1) for x in (p1_rows, p2_rows))
        K = a.shape[1]
        wp = np.ascontiguousarray(np.stack([a, b], axis=1))  # [F][2][K]
        dts = np.broadcast_to(np.asarray(T, dtype=np.float64), (K,)).reshape(1, K)
        flags = np.full((2, K), USE_POS | USE_VEL | USE_ACC, np.uint8)
        return self.solve_traj(wp, dts=dts, control=control, wp_flags=flags)

    # ---- the persistent node table (include/mplx_table.h; table.py): relax successor lists, emit the next frontier
    def alloc_table(self, capacity, slots_log2=0, n_queries=1):
        from .table import NodeTable
        return NodeTable(self, capacity, slots_log2, n_queries)

    def alloc_table_frontier(self, capacity):
        from .table import TableFrontier
        return TableFrontier(self, capacity)

    def cost_to_come(self, starts, g=None, g_max=float("inf"), max_rounds=None, capacity=1 << 16, lists_stride=None,
                     max_frontier=None):
        """A label-correcting sweep from `starts` ([4D+2][n] or one state; cost-to-come g, default 0): seed, then while
        the frontier is not empty expand it, relax its lists against the table, and go on with the nodes whose g fell.
        Nodes with g > g_max are never created.  Everything stays on the device; the host reads one 8-byte count per
        round.  Lists and the two frontiers are allocated once, for max_frontier nodes (default: capacity, which no
        frontier can exceed).  Returns (table, rounds): rounds = relax calls made; at the fixed point (the last one left
        an empty frontier) table.download()["g"] is the exact cost-to-come of every reachable lattice state within
        g_max.  A table that ran out of nodes, probe length or frontier raises."""
        from .table import NodeTable, TableFrontier
        self._flush()
        fcap = int(capacity if max_frontier is None else max_frontier)
        tab = NodeTable(self, capacity)
        cur, nxt = TableFrontier(self, fcap), TableFrontier(self, fcap)
        lists = self.alloc_lists(fcap, want_state=True, stride=lists_stride)
        try:
            def check(where):
                status = tab.stats()[1]  # (the stream is idle: no copy, no wait)
                if status:
                    raise RuntimeError("cost_to_come: table status %d %s (1 nodes full, 2 probe full, 4 frontier full): "
                                       "raise capacity / max_frontier" % (status, where))
            count = tab.seed(starts, g, frontier=cur)
            check("after seeding")
            rounds = 0
            while count > 0 and (max_rounds is None or rounds < max_rounds):
                self.expand_lists_resident(cur, lists, n_nodes=count)
                count = tab.relax(lists, cur.id, cur.g, g_max, frontier=nxt, n_nodes=count)
                rounds += 1
                check("in round %d" % rounds)
                cur, nxt = nxt, cur
        except Exception:
            tab.free()
            raise
        finally:
            for b in (cur, nxt, lists):
                b.free()
        return tab, rounds

    # ---- the open set of a table (include/mplx_open.h; search.py): goal-directed search on the device
    def alloc_open(self, table):
        from .search import OpenSet
        return OpenSet(self, table)

    def alloc_field(self):
        """An empty search.GoalField (include/mplx_field.h): build(goal_rows, tol_pos) makes it the grid distance of
        every cell to a goal region; the `field` of search / search_many, or OpenSet.set_field."""
        from .search import GoalField
        return GoalField(self)

    def search(self, start, goal_row, eps=1.0, delta=None, g_max=float("inf"), max_rounds=None, max_expand=None,
               capacity=1 << 16, max_frontier=None, lists_stride=None, sight=True, tol_pos=0.5, tol_vel=-1.0, tol_acc=-1.0,
               tol_yaw=-1.0, w=None, v_max=None, start_g=0.0, prior=None, avoid=None, t0=0.0, radius=None, ignore_group=-1,
               time_keys=None, wait=False, park_goal=False, field=None, field_of_query=None, heur=None, best=None,
               body=None, body_samples=4):
        """A goal-directed search from `start` (one 4D+2 state) to the goal region of `goal_row` that stays on the
        device: set_goal, seed, push; then per round one select (the round's only read-back, 48 bytes), and while it
        selects: expand the selection, relax its lists against the table, push the nodes whose g fell.  Keys are
        f = g + eps * h with the default heuristic; a select takes every open node with f <= f_min + delta (default
        delta: w * dt, the time term every edge costs at least; 0 is A*'s one-key-at-a-time order, +inf the
        label-correcting sweep) and announces the goal once no open key is below the best goal-region node's.
        sight: a goal-region node also needs a free line of sight to the goal (env_map::is_goal's ray trace).
        Nodes with g > g_max are never created.  Lists and the selection frontier are allocated for max_frontier nodes
        (default: capacity); a larger selection is taken in id order, the rest stays open.  Returns a SearchResult
        (search.py) that owns the table and the open set.  A table that ran out of nodes or probe length raises.
        start_g: the cost-to-come the start is seeded with (what a SearchResult.replan from a node with that g is
        compared against).  result.replan(...) plans again on the same table after a move or a map edit.
        prior: a search.Prior (e.g. another result's as_prior()): the heuristic follows the prior trajectory at the
        node's own time and the goal moves to the prior's end (include/mplx_prior.h).
        avoid: a search.Reservations (alloc_reservations): every round checks its lists against the reserved trajectories
        between the expansion and the relax, and the edges that come closer to one than radius + its radius cost +inf
        (include/mplx_reserve.h).  The robot starts at t0 on the table's clock (its clock is t0 + t, so `start` must
        have t = 0), has `radius` and ignores the reservations of ignore_group (-1: none).  time_keys (default: on with
        avoid, else off): a node is a (lattice state, time) pair (mplx_table_set_time_keys) -- what waiting for a moving
        obstacle to pass needs.  Without avoid and time keys the search issues exactly the calls it always did.  A
        result of a search with avoid or time keys replans with replan_timed() (include/mplx_replan_timed.h), not replan().
        wait=True (needs time keys, else ValueError): every round appends the wait edge -- the all-zero control from a
        state it leaves where it is, which the expansion drops -- to its lists before the check (include/mplx_wait.h).
        park_goal=True (needs avoid, else ValueError): after every push a goal-region node at which the robot could not
        stay to the table's horizon loses its goal bit (mplx_reserve_park_device, include/mplx_reserve.h) and is
        expanded like any other.  With both off the search issues exactly the calls it issued before they existed.
        field: None -- the calls of a search without one.  True: a goal distance field (include/mplx_field.h) is built for
        the goal, set after the goal and freed with the result: the heuristic becomes w * max(Linf, res * (dist - 1)) / v_max,
        which sees walls and dead ends and stays admissible.  A search.GoalField (alloc_field; with field_of_query, default
        [0]) is used as given and not freed.  field together with prior is a ValueError.
        heur: None -- the default heuristic and the calls of a search without the argument.  "robust": the pushes take
        the dynamics-aware heuristic (include/mplx_heur.h; OpenSet.set_heur): the cost of the unconstrained connection to
        the goal STATE minimised over the arrival time, never below the default; with a field the larger of the two.  A
        replan keeps the mode.  heur together with prior is a ValueError.
        best: None -- the calls of a search without the argument.  k >= 1: a round expands only the k smallest keys among
        the open nodes with f <= f_min + delta (ties by id; include/mplx_best.h), so delta=inf with best=k is a priority
        queue that hands out k nodes a round.  It does nothing to optimality: the stopping rule is unchanged, the goal is
        announced once no open key is below the best goal-region node's.  Without max_frontier the selection frontier and
        the lists are allocated for min(capacity, best) nodes.  A replan keeps it.
        body: None -- the calls of a search without the argument.  A search.Body (alloc_body, filled): every round checks
        its lists against the body's cloud after the wait edges and the reservation check and before the relax
        (include/mplx_body.h): an edge along which the ellipsoid, tilted as the edge's acceleration tilts it, touches a
        point at one of body_samples + 1 samples, or has a bad attitude there, costs +inf.  One body serves all queries;
        start and goal are checked only through their edges; the cloud must not be filled again while the result lives
        (improve and anytime raise if it was); replan / replan_timed of such a result raise; shortcut and smooth are not
        body-checked (Body.check_poly reports)."""
        from .search import run_search
        return run_search(self, start, goal_row, prior=prior, eps=eps, delta=delta, g_max=g_max, max_rounds=max_rounds,
                          max_expand=max_expand, capacity=capacity, max_frontier=max_frontier, lists_stride=lists_stride,
                          sight=sight, tol_pos=tol_pos, tol_vel=tol_vel, tol_acc=tol_acc, tol_yaw=tol_yaw, w=w, v_max=v_max,
                          start_g=start_g, avoid=avoid, t0=t0, radius=radius, ignore_group=ignore_group, time_keys=time_keys,
                          wait=wait, park_goal=park_goal, field=field, field_of_query=field_of_query, heur=heur, best=best,
                          body=body, body_samples=body_samples)

    def search_many(self, starts, goal_rows, eps=1.0, delta=None, g_max=float("inf"), max_rounds=None, max_expand=None,
                    capacity=1 << 16, max_frontier=None, lists_stride=None, sight=True, tol_pos=0.5, tol_vel=-1.0,
                    tol_acc=-1.0, tol_yaw=-1.0, w=None, v_max=None, start_g=0.0, priors=None, avoid=None, t0=0.0, radius=None,
                    ignore_group=-1, time_keys=None, wait=False, park_goal=False, field=None, field_of_query=None, heur=None,
                    best=None, body=None, body_samples=4):
        """Q searches of EnvMap.search at once, sharing every launch of a round (include/mplx_multi.h): starts
        [4D+2][Q], goal_rows [Q][4D+2], query q from starts[:, q] to the goal region of goal_rows[q].  One table of
        `capacity` nodes and one open set hold all of them; a round selects, expands, relaxes and pushes the union of
        what the queries select, and reads Q results back.  The loop goes on while any query selects; max_expand counts
        all queries together.  As long as no selection is cut at max_frontier every query does exactly what its own
        EnvMap.search does.  Returns a MultiSearchResult (search.py) that owns the table and the open set.  start_g: one
        cost-to-come for every start, or [Q].  priors: [Q] search.Prior or None (no prior for that query), e.g. another
        result's as_priors(): one mplx_open_set_priors_device for all of them (include/mplx_prior.h).
        avoid, t0, radius, ignore_group (one value for all queries or [Q]), time_keys, wait and park_goal: as EnvMap.search takes them;
        every query has its own start on the clock, radius and ignored group, and one check serves them all.
        field: as EnvMap.search takes it; True builds one field per DISTINCT goal row (the delay candidates of one robot
        share one); a GoalField is used with field_of_query [Q] (default: query q uses field q; -1: the default heuristic).
        heur: as EnvMap.search takes it; every query's own goal is the one its rows are measured against.
        best: as EnvMap.search takes it, per query: every query selects its own k smallest keys, and without max_frontier
        the selection frontier and the lists are allocated for min(capacity, best * Q) nodes, which no round can exceed.
        Optimality is untouched: every query's stopping rule is the one it had.
        body, body_samples: as EnvMap.search takes them; one body and one check serve all queries."""
        from .search import run_search_many
        return run_search_many(self, starts, goal_rows, priors=priors, eps=eps, delta=delta, g_max=g_max, max_rounds=max_rounds,
                               max_expand=max_expand, capacity=capacity, max_frontier=max_frontier, lists_stride=lists_stride,
                               sight=sight, tol_pos=tol_pos, tol_vel=tol_vel, tol_acc=tol_acc, tol_yaw=tol_yaw, w=w,
                               v_max=v_max, start_g=start_g, avoid=avoid, t0=t0, radius=radius, ignore_group=ignore_group,
                               time_keys=time_keys, wait=wait, park_goal=park_goal, field=field, field_of_query=field_of_query,
                               heur=heur, best=best, body=body, body_samples=body_samples)

    def _heur_goal(self, goal_row, goal_control, w, v_max):
        goal = np.ascontiguousarray(goal_row, dtype=np.float64)
        if goal.shape != (self.n_fields,):
            raise ValueError("goal_row must have %d entries" % self.n_fields)
        g = _abi.GoalSpec()
        g.goal, g.control, g.goal_control = goal.ctypes.data, int(self._p.control), int(goal_control)
        g.w = float(self._p.w if w is None else w)
        g.v_max = float(self._p.v_max if v_max is None else v_max)
        g.tol_pos, g.tol_vel, g.tol_acc, g.tol_yaw = 0.0, -1.0, -1.0, -1.0
        return g, goal

    def heur_eval(self, states, goal_row, mode="robust", goal_control=0, w=None, v_max=None):
        """mplx_heur_eval (include/mplx_heur.h): get_heur of the state columns `states` ([4D+2][K], or one state) against
        `goal_row` under `mode` ("robust", or "default"; "reference" is the host planner's and refused here), with the
        context's control flag, w and v_max unless given.  Returns h [K]."""
        self._flush()
        st = np.ascontiguousarray(np.asarray(states, dtype=np.float64).reshape(self.n_fields, -1))
        K = st.shape[1]
        g, keep = self._heur_goal(goal_row, goal_control, w, v_max)
        out = np.zeros(K)
        _abi.check(self._ctx, _abi.lib().mplx_heur_eval(self._ctx, C.byref(g), _abi.heur_mode(mode), st.ctypes.data, K, K,
                                                        out.ctypes.data))
        return out

    def heur_eval_resident(self, states, goal_row, out, n=None, stride=None, mode="robust", goal_control=0, w=None, v_max=None):
        """mplx_heur_eval_device: the same on resident rows -- `states` a TableFrontier (its state rows, n = its capacity
        unless given) or a device buffer [4D+2][stride]; `out` a device buffer of n doubles.  Asynchronous."""
        self._flush()
        if hasattr(states, "state_stride"):  # a TableFrontier
            ptr, stride, n = states.state.ptr, states.state_stride, (states.capacity if n is None else n)
        else:
            ptr = _device_ptr(states)
            if stride is None:
                raise ValueError("heur_eval_resident: a device buffer needs its stride")
            n = stride if n is None else n
        g, keep = self._heur_goal(goal_row, goal_control, w, v_max)
        _abi.check(self._ctx, _abi.lib().mplx_heur_eval_device(self._ctx, C.byref(g), _abi.heur_mode(mode), ptr, int(n),
                                                               int(stride), _device_ptr(out)))

    def alloc_reservations(self, trajs, step, n_steps=None, t0=None, radius=None, group=None, park=True):
        """A reservation table on the device (include/mplx_reserve.h; search.Reservations): the positions of the
        trajectories `trajs` -- a PolyTrajSet, or (starts, actions) chains as traj_conflicts takes them -- at the instants
        i * step of a common clock, with t0 / radius / group / park as conflicts() takes them.  n_steps=None covers
        max(t0 + total), as conflicts() does.  The `avoid` of search / search_many."""
        from .search import Reservations
        return Reservations(self, trajs, step, n_steps, t0, radius, group, park)

    def alloc_body(self, r, h, g=9.81, tilt_max=None):
        """An ellipsoid body and its obstacle point cloud on the device (include/mplx_body.h; search.Body): radius r across
        the thrust axis, half-height h along it, the axis along acc + g e_z, tilt_max the largest tilt in radians (None:
        any attitude whose thrust points up).  fill() / fill_resident() / fill_map() give it the cloud.  The `body` of
        search / search_many."""
        from .search import Body
        return Body(self, r, h, g, tilt_max)

    def anytime(self, result, schedule, max_expand=None, avoid=None):
        """search.anytime: improve a SearchResult / MultiSearchResult of this EnvMap through a non-increasing schedule of eps
        on the tree it has paid for (include/mplx_anytime.h); returns (final_result, stages)."""
        from .search import anytime
        return anytime(result, schedule, max_expand=max_expand, avoid=avoid)

    def synchronize(self):
        _abi.check(self._ctx, _abi.lib().mplx_synchronize(self._ctx))

    def timer_begin(self):
        _abi.check(self._ctx, _abi.lib().mplx_timer_begin(self._ctx))

    def timer_end(self):
        ms = C.c_float()
        _abi.check(self._ctx, _abi.lib().mplx_timer_end(self._ctx, C.byref(ms)))
        return ms.value

    def set_lists_route(self, route):
        """Force the kernel behind expand_lists* ("auto", "dense", "tile", "grid"); diagnostic."""
        code = {"auto": _abi.ROUTE_AUTO, "dense": _abi.ROUTE_DENSE, "tile": _abi.ROUTE_TILE,
                "grid": _abi.ROUTE_GRID}[route] if isinstance(route, str) else int(route)
        _abi.check(self._ctx, _abi.lib().mplx_set_lists_route(self._ctx, code))

    def last_lists_route(self):
        code = _abi.lib().mplx_last_lists_route(self._ctx)
        return {_abi.ROUTE_AUTO: "none", _abi.ROUTE_DENSE: "dense", _abi.ROUTE_TILE: "tile",
                _abi.ROUTE_GRID: "grid"}[code]

    def debug_store_model(self, lists, n_nodes=None):
        """DIAGNOSTIC: the list stores of an expansion launch alone, into `lists` (mplx_debug_store_model): every node's first
        count[k] entries of every row, unspecified values.  Overwrites the successor entries; asynchronous."""
        self._flush()
        s = lists.c_struct()
        _abi.check(self._ctx, _abi.lib().mplx_debug_store_model(self._ctx, C.byref(s), lists.n_nodes if n_nodes is None else int(n_nodes)))
        if hasattr(lists, "zero_rows"):  # it leaves alone the rows the last launch skipped and writes junk into all others
            lists.zero_rows &= self.last_lists_zero_rows()

    def last_lists_zero_rows(self):
        """Bit mask of the state rows the last expand_lists* call of this context did not store to
        (mplx_last_lists_zero_rows): 0 unless the lists carried a mask and the GRID route ran."""
        return int(_abi.lib().mplx_last_lists_zero_rows(self._ctx))

    def last_grid_kernel(self):
        """Which kernel of the GRID route the last expand_lists* call ran: "lex" (expand_lex_kernel.hip: lexicographic
        control table, no yaw, occupancy map), "grid" (expand_grid_kernel.hip), "pair" (expand_pair_kernel.hip: yaw controls on
        a potential map over a pre-screened frontier, two nodes per wave), "none" (another route)."""
        return {0: "none", 1: "grid", 2: "lex", 3: "pair"}[_abi.lib().mplx_last_grid_kernel(self._ctx)]

    def last_identity_form(self):
        """Which form of the node-identity pass the last post_lists / post_packed call with canon ran: "table" (in HBM, small
        batches), "claimed" (partition into buckets of fixed capacity), "exact" (partition by histograms),
        "claimed+exact" (a bucket overflowed: the exact form ran after the claimed one).  Same canon[] from all."""
        return {0: "table", 1: "claimed", 2: "exact", 3: "claimed+exact"}[_abi.lib().mplx_last_identity_form(self._ctx)]

    def yaw_pin_stats(self):
        """(nodes re-expanded with the host libm's trig values, fix passes launched) since the context was made."""
        a, b = C.c_int64(), C.c_int64()
        _abi.check(self._ctx, _abi.lib().mplx_yaw_pin_stats(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def service(self, mode=-1):
        """The resident kernel behind small synchronous batches (include/mplx.h, mplx_service): mode 1 on, 0 off,
        -1 unchanged; returns dict(requests, launches, failures, resident)."""
        st = (C.c_int64 * 4)()
        _abi.check(self._ctx, _abi.lib().mplx_service(self._ctx, int(mode), st))
        return {"requests": st[0], "launches": st[1], "failures": st[2], "resident": bool(st[3])}

    def selftest_math(self, op, a, b=None):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = a if b is None else np.ascontiguousarray(b, dtype=np.float64)
        out = np.empty_like(a)
        _abi.check(self._ctx, _abi.lib().mplx_selftest_math(self._ctx, int(op), a.ctypes.data, b.ctypes.data,
                                                             out.ctypes.data, a.size))
        return out
