"""Device allocations and the fixed-shape output rows of the C ABI (the mplx_*_out structures of include/).

A rows class declares its buffers ONCE, as the class-level table FIELDS; _Rows makes the allocation, the C structure,
download(), free() and fill() from it, and the host twin of the same structure that the synchronous (host-pointer) calls
hand to the library: Cls.host(env, sizes...) -> (rows, structure).  Stride members, which are not buffers, are the short
_strides hook of each class.
"""
import ctypes as C
import math

import numpy as np

from . import _abi


class DeviceArray:
    """An HBM allocation made through the C ABI (mplx_device_alloc)."""

    def __init__(self, env, nbytes):
        self._env = env
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _abi.check(env._ctx, _abi.lib().mplx_device_alloc(env._ctx, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, host):
        host = np.ascontiguousarray(host)
        assert host.nbytes <= self.nbytes
        _abi.check(self._env._ctx, _abi.lib().mplx_memcpy_h2d(self._env._ctx, self.ptr, host.ctypes.data, host.nbytes))

    def download(self, dtype, shape, offset=0):
        """Copy `shape` elements of `dtype` starting `offset` BYTES into the allocation back to the host."""
        out = np.empty(shape, dtype=dtype)
        assert int(offset) + out.nbytes <= self.nbytes
        _abi.check(self._env._ctx, _abi.lib().mplx_memcpy_d2h(self._env._ctx, out.ctypes.data, self.ptr + int(offset),
                                                               out.nbytes))
        return out

    def free(self):
        if self.ptr and self._env._ctx:
            _abi.lib().mplx_device_free(self._env._ctx, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _alloc(env, nbytes, alloc=None):
    """An HBM allocation for the engine: through the C ABI by default, or from `alloc(nbytes)` -- any object with
    .ptr / .nbytes / .download / .free, e.g. shard.TorchArray, so that torch.distributed can move the same memory."""
    return DeviceArray(env, nbytes) if alloc is None else alloc(int(nbytes))


class DeviceArrayView:
    """A raw device pointer the engine did not allocate (e.g. a field of a ready C struct): read-back helper."""

    def __init__(self, env, ptr):
        self._env, self.ptr = env, int(ptr)

    def download_i64(self, index):
        out = np.empty(1, dtype=np.int64)
        _abi.check(self._env._ctx, _abi.lib().mplx_memcpy_d2h(self._env._ctx, out.ctypes.data, self.ptr + 8 * int(index), 8))
        return out[0]


def _device_ptr(buf):
    """The device address of a DeviceArray (or anything with .ptr) or of a torch tensor (data_ptr())."""
    if hasattr(buf, "ptr"):
        return int(buf.ptr)
    if hasattr(buf, "data_ptr"):
        return int(buf.data_ptr())
    raise TypeError("need a device buffer with .ptr or .data_ptr(), got %r" % type(buf))


u8, i32, f64, u64 = np.dtype(np.uint8), np.dtype(np.int32), np.dtype(np.float64), np.dtype(np.uint64)


def _f(name, dtype, shape=lambda s, n: (n,), on=None, key=None, member=None, group="out", show=None):
    """One buffer of a rows class: the attribute, the numpy dtype, shape(rows, n) for n entries, on(rows): whether the
    buffer exists (None: always), key: its name in download() and member: in the C structure (default: the attribute),
    group: which of the class's structures it belongs to, show(rows): whether download() returns it (None: always)."""
    return name, dtype, shape, on, key or name, member or name, group, show


class _Rows:
    """HBM-resident rows of one output structure for `self.n` entries, from FIELDS.  A buffer holds one element at least
    (an empty set still has addresses to give).  The subclass's __init__ sets the sizes and calls _alloc(env)."""

    STRUCT = None  # the _abi structure of c_struct()
    FIELDS = ()
    _on_host = False

    def _alloc(self, env):
        n = max(self.n, 1)
        self._ptrs = {}  # group -> [(member, address)]: what c_struct() sets, made once
        for name, dt, shape, on, key, member, group, show in self.FIELDS:
            buf = None
            if on is None or on(self):
                if self._on_host:
                    buf = np.zeros(shape(self, self.n), dt)
                    ptr = buf.ctypes.data
                else:
                    buf = DeviceArray(env, max(math.prod(shape(self, n)), 1) * dt.itemsize)
                    ptr = buf.ptr
                self._ptrs.setdefault(group, []).append((member, ptr))
            setattr(self, name, buf)

    def _fill(self, s, group="out"):
        for member, ptr in self._ptrs.get(group, ()):
            setattr(s, member, ptr)
        return s

    def _strides(self, s):
        """The members of the structure that are not buffers."""

    def c_struct(self):
        s = self._fill(self.STRUCT())
        self._strides(s)
        return s

    def _all(self):
        return [b for b in (getattr(self, f[0]) for f in self.FIELDS) if b is not None]

    def fill(self, byte):
        """Every row set to `byte` (to see afterwards what a call wrote)."""
        for b in self._all():
            _abi.check(b._env._ctx, _abi.lib().mplx_memset(b._env._ctx, b.ptr, int(byte), b.nbytes))

    def download(self):
        """Entries a call did not own hold whatever the buffers held."""
        return {key: getattr(self, name).download(dt, shape(self, self.n))
                for name, dt, shape, on, key, member, group, show in self.FIELDS
                if getattr(self, name) is not None and (show is None or show(self))}

    def free(self):
        if not self._on_host:
            for b in self._all():
                b.free()
        self._ptrs = {}

    # ---- the host twin: the same structure over numpy arrays of zeros, for the synchronous calls
    @classmethod
    def _host(cls, env, *args, **kw):
        h = cls.__new__(cls)
        h._on_host = True
        h.__init__(env, *args, **kw)
        return h

    def _host_rows(self, group=None):
        """The arrays by download key: those of one structure, or (None) those download() would return."""
        return {key: getattr(self, name) for name, dt, shape, on, key, member, grp, show in self.FIELDS
                if getattr(self, name) is not None and (grp == group if group else (show is None or show(self)))}

    @classmethod
    def host(cls, env, *args, **kw):
        """(rows, structure) with the constructor's arguments: the dict download() would return, as arrays of zeros on
        the host, and the structure that points at them.  Keep `rows` for as long as the structure is in use."""
        h = cls._host(env, *args, **kw)
        return h._host_rows(), h.c_struct()


class Rollouts(_Rows):
    """HBM-resident output rows of n rollouts (mplx_rollout_out)."""

    STRUCT = _abi.RolloutOut
    FIELDS = (_f("status", u8), _f("steps", i32), _f("cost", f64), _f("prefix_cost", f64),
              _f("end_state", f64, lambda s, n: (s.n_fields, n), lambda s: s.want_end), _f("end_hash", u64, on=lambda s: s.want_end),
              _f("end_heur", f64, on=lambda s: s.want_goal_rows), _f("end_flags", u8, on=lambda s: s.want_goal_rows))

    def __init__(self, env, n_rollouts, want_end=True, want_goal_rows=False):
        self.n, self.n_fields = int(n_rollouts), env.n_fields
        self.want_end, self.want_goal_rows = bool(want_end), bool(want_goal_rows)
        self._alloc(env)

    def _strides(self, s):
        s.end_stride = self.n


class Rays(_Rows):
    """HBM-resident output rows of n rays (mplx_ray_out); cells only with cell_cap > 0."""

    STRUCT = _abi.RayOut
    FIELDS = (_f("status", u8), _f("n_cells", i32, on=lambda s: s.want_counts), _f("first_hit", i32, on=lambda s: s.want_counts),
              _f("cells", i32, lambda s, n: (n, s.cell_cap), lambda s: s.cell_cap > 0))

    def __init__(self, env, n, cell_cap=0, want_counts=True):
        self.n, self.cell_cap, self.want_counts = int(n), int(cell_cap), bool(want_counts)
        self._alloc(env)

    def _strides(self, s):
        s.cell_cap = self.cell_cap


class TrajInfo(_Rows):
    """HBM-resident rows of mplx_traj_info_out for n trajectories of up to `horizon` segments."""

    STRUCT = _abi.TrajInfoOut
    FIELDS = (_f("status", u8), _f("n_segs", i32), _f("total_time", f64), _f("effort", f64, lambda s, n: (5, n)),
              _f("seg_state", f64, lambda s, n: (s.n_fields, s.horizon + 1, n), lambda s: s.want_states))

    def __init__(self, env, n, horizon, want_states=False):
        self.n, self.horizon, self.n_fields, self.want_states = int(n), int(horizon), env.n_fields, bool(want_states)
        self._alloc(env)

    def _strides(self, s):
        s.effort_stride = s.seg_stride = self.n


class TrajSamples(_Rows):
    """HBM-resident sample rows (mplx_traj_sample_out): [4D+3][n_stride][sample_stride] float64, and status [n]."""

    STRUCT = _abi.TrajSampleOut
    FIELDS = (_f("out", f64, lambda s, n: (s.rows, s.n_stride, s.sample_stride), key="samples"), _f("status", u8))

    def __init__(self, env, n, count, n_stride=None, sample_stride=None):
        self.n, self.count, self.rows = int(n), int(count), 4 * env.dim + 3
        self.n_stride = self.n if n_stride is None else int(n_stride)
        self.sample_stride = self.count if sample_stride is None else int(sample_stride)
        self._alloc(env)

    def _strides(self, s):
        s.row_stride, s.sample_stride = self.n_stride * self.sample_stride, self.sample_stride


class TrajTraverse(_Rows):
    """HBM-resident rows of mplx_traj_traverse_out for n trajectories."""

    STRUCT = _abi.TrajTraverseOut
    FIELDS = (_f("status", u8), _f("cost", f64), _f("n_samples", i32), _f("n_cells", i32), _f("stop_sample", i32))

    def __init__(self, env, n):
        self.n = int(n)
        self._alloc(env)


class SolveOut(_Rows):
    """HBM-resident rows of mplx_solve_out for n problems of up to w_max waypoints with smoothing order so.  Rows the
    solve did not own (failed problems, segments past S_k) hold whatever the buffers held."""

    STRUCT = _abi.SolveOut
    FIELDS = (_f("status", u8), _f("n_segs", i32), _f("total_time", f64),
              _f("coeff", f64, lambda s, n: (s.w_max - 1, 2 * (s.so + 1), s.dim, n)),
              _f("dts", f64, lambda s, n: (s.w_max - 1, n), member="dts_out"), _f("yaw_coeff", f64, lambda s, n: (s.w_max - 1, 2, n)),
              _f("taus", f64, lambda s, n: (s.w_max, n)))

    def __init__(self, env, n, w_max, so):
        self.n, self.w_max, self.so, self.dim = int(n), int(w_max), int(so), env.dim
        self.rows = (self.w_max - 1) * 2 * (self.so + 1) * self.dim
        self._alloc(env)

    def _strides(self, s):
        s.coeff_stride = s.dts_out_stride = s.yaw_stride = s.taus_stride = self.n


class LoadOut(_Rows):
    """HBM-resident rows of mplx_poly_load_out for n problems of up to w_max - 1 segments.  Rows the load did not own
    (failed problems, taus past S_k) hold whatever the buffers held."""

    STRUCT = _abi.PolyLoadOut
    FIELDS = (_f("status", u8), _f("n_segs", i32), _f("total_time", f64), _f("taus", f64, lambda s, n: (s.w_max, n)))

    def __init__(self, env, n, w_max):
        self.n, self.w_max = int(n), int(w_max)
        self._alloc(env)

    def _strides(self, s):
        s.taus_stride = self.n


class PolyLimits(_Rows):
    """HBM-resident rows of mplx_limits_out for n trajectories.  Entries of failed problems hold whatever the buffers held."""

    STRUCT = _abi.LimitsOut
    FIELDS = tuple(_f(k, f64, lambda s, n: (s.dim, n)) for k in ("max_vel", "max_acc", "max_jrk")) + (
        _f("exceed", u8), _f("valid", u8), _f("first_bad", i32))

    def __init__(self, env, n):
        self.n, self.dim = int(n), env.dim
        self._alloc(env)

    def _strides(self, s):
        s.max_stride = self.n


class LambdaRows(_Rows):
    """HBM-resident rows of mplx_lambda_out / mplx_scale_down_out for n problems of up to w_max waypoints, and of
    mplx_tau_out when count > 0 ([n][count] each)."""

    STRUCT = _abi.LambdaOut
    FIELDS = (_f("status", u8), _f("n_lseg", i32), _f("total", f64), _f("Ts", f64, lambda s, n: (s.w_max, n)),
              _f("segs", f64, lambda s, n: (8, 8, n))) + tuple(
        _f(k, dt, group="down") for k, dt in (("scaled", u8), ("max_l", f64), ("t_lo", f64), ("t_hi", f64))) + tuple(
        _f(k, dt, lambda s, n: (n, s.count), key=key, group="tau", show=lambda s: s.count > 0)
        for k, dt, key in (("tau", f64, None), ("lam", f64, "lambda"), ("lam_dot", f64, "lambda_dot"), ("found", u8, None)))

    def __init__(self, env, n, w_max, count=0):
        self.n, self.w_max, self.count = int(n), int(w_max), int(count)
        self._alloc(env)

    def _strides(self, s):
        s.ts_stride = s.seg_stride = self.n

    def c_down(self):
        s = self._fill(_abi.ScaleDownOut(), "down")
        s.lam = self.c_struct()
        return s

    def c_tau(self):
        s = self._fill(_abi.TauOut(), "tau")
        s.stride = self.count
        return s


class Conflicts(_Rows):
    """HBM-resident rows of mplx_conflict_out for n trajectories; want_pairs: pair_first [n][n] int32 as well."""

    STRUCT = _abi.ConflictOut
    FIELDS = (_f("first_step", i32), _f("first_partner", i32), _f("min_d2", f64), _f("status", u8),
              _f("pair_first", i32, lambda s, n: (n, n), lambda s: s.want_pairs))

    def __init__(self, env, n, want_pairs=False):
        self.n, self.want_pairs = int(n), bool(want_pairs)
        self._alloc(env)

    def _strides(self, s):
        if self.want_pairs:
            s.pair_stride = self.n

    def result(self, step):
        """The rows as a ConflictResult (synchronize() first)."""
        d = self.download()
        return ConflictResult(step, d["first_step"], d["first_partner"], d["min_d2"], d["status"], d.get("pair_first"))


class ConflictResult:
    """What conflicts() returns, per trajectory over the pairs charged to it (include/mplx_conflict.h): first_step (the
    first instant with a conflict, -1: none), first_time (first_step * step; NaN: none), partner (the smallest index it
    conflicts with at that instant, -1), min_d2 and min_dist = sqrt(min_d2) (the closest approach to a charged partner
    while both are active; inf: none), status (the set's bits | CONFLICT_BAD_INPUT; a trajectory with any bit is
    excluded: -1, -1, inf), and pairs [K][K] (want_pairs; the first instant at which two trajectories conflict regardless
    of rank, symmetric, -1: never), else None."""

    def __init__(self, step, first_step, partner, min_d2, status, pairs=None):
        self.step = float(step)
        self.first_step, self.partner, self.min_d2, self.status, self.pairs = first_step, partner, min_d2, status, pairs
        self.first_time = np.where(first_step >= 0, first_step.astype(np.float64) * self.step, np.nan)
        self.min_dist = np.sqrt(min_d2)

    @property
    def charged(self):
        """[K] bool: the trajectory has a conflict charged to it."""
        return self.first_step >= 0

    def __repr__(self):
        return "ConflictResult(%d of %d trajectories in conflict)" % (int(self.charged.sum()), len(self.first_step))
