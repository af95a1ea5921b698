"""The fixed-shape output rows of env.py against the structures of include/: per class the byte size of every buffer, which
pointer members of the _abi structure are set, every stride member, and the keys, dtypes and shapes of download().  The
expected values are written out from the headers (include/mplx_rollout.h, mplx_ray.h, mplx_traj.h, mplx_solve.h,
mplx_limits.h, mplx_scale.h, mplx_conflict.h); nothing here is computed from the class under test.  No GPU and no library
call: DeviceArray is replaced by a numpy-backed stand-in.  Where a class has a host twin (Cls.host(env, sizes...) -> (rows,
structure)) the same is asserted of it."""
import ctypes as C
import sys

import numpy as np
import pytest

from motion_primitive_library_amd import _abi
from motion_primitive_library_amd import env as E

u8, i32, f64, u64 = np.uint8, np.int32, np.float64, np.uint64
N, W_MAX, HORIZON, COUNT, CELL_CAP = 3, 4, 2, 2, 5


class FakeArray:
    """.ptr / .nbytes / download / free of a DeviceArray, on host memory."""

    def __init__(self, env, nbytes):
        self.nbytes = int(nbytes)
        self._mem = np.zeros(self.nbytes, np.uint8)
        self.ptr = self._mem.ctypes.data

    def download(self, dtype, shape, offset=0):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert int(offset) + n <= self.nbytes, "download past the end of the buffer"
        return self._mem[int(offset):int(offset) + n].view(dtype).reshape(shape).copy()

    def free(self):
        self.ptr = None


class FakeEnv:
    _ctx = None

    def __init__(self, dim):
        self.dim, self.n_fields = dim, 4 * dim + 2


def pointer_members(struct):
    return [name for name, tp in struct._fields_ if tp is C.c_void_p]


def check(monkeypatch, name, dim, args, kw, nbytes, members, strides, download, struct=lambda o: o.c_struct(), host=True):
    """nbytes: attribute -> bytes, or None for a buffer that must not exist.  members: pointer member of the structure ->
    (attribute, download key), or None where it must stay null; every pointer member must be named.  strides: member ->
    value.  download: key -> (dtype, shape)."""
    cls = getattr(E, name)
    monkeypatch.setattr(sys.modules[cls.__module__], "DeviceArray", FakeArray)
    env = FakeEnv(dim)
    obj = cls(env, *args, **kw)
    for attr, nb in nbytes.items():
        buf = getattr(obj, attr)
        assert (buf is None) if nb is None else (buf is not None and buf.nbytes == nb), (name, attr, nb, getattr(buf, "nbytes", None))
    s = struct(obj)
    assert set(pointer_members(s)) == set(members), (name, "every pointer member has an expectation")
    for member, src in members.items():
        got = getattr(s, member)
        assert got == (None if src is None else getattr(obj, src[0]).ptr), (name, member)
    for member, v in strides.items():
        assert getattr(s, member) == v, (name, member, getattr(s, member), v)
    d = obj.download()
    assert set(d) == set(download), (name, sorted(d))
    for key, (dt, shape) in download.items():
        assert d[key].dtype == dt and d[key].shape == shape, (name, key, d[key].dtype, d[key].shape)
    if host and hasattr(cls, "host"):  # the host twin: the same keys, dtypes, shapes, members and strides
        rows, hs = cls.host(env, *args, **kw)
        assert type(hs) is type(obj.c_struct())
        assert set(rows) == set(download), (name, "host", sorted(rows))
        for key, (dt, shape) in download.items():
            assert rows[key].dtype == dt and rows[key].shape == shape and not rows[key].any(), (name, "host", key)
        for member, src in members.items():
            assert getattr(hs, member) == (None if src is None else rows[src[1]].ctypes.data), (name, "host", member)
        for member, v in strides.items():
            assert getattr(hs, member) == v, (name, "host", member)
    obj.free()


def same(*names):
    return {k: (k, k) for k in names}


@pytest.mark.parametrize("dim,state_bytes", [(2, 240), (3, 336)])  # [4D+2][3] float64
@pytest.mark.parametrize("want_end", [True, False])
@pytest.mark.parametrize("want_goal_rows", [True, False])
def test_rollouts(monkeypatch, dim, state_bytes, want_end, want_goal_rows):
    nbytes = {"status": 3, "steps": 12, "cost": 24, "prefix_cost": 24, "end_state": state_bytes if want_end else None,
              "end_hash": 24 if want_end else None, "end_heur": 24 if want_goal_rows else None, "end_flags": 3 if want_goal_rows else None}
    members = same("status", "steps", "cost", "prefix_cost")
    members.update(same("end_state", "end_hash") if want_end else {"end_state": None, "end_hash": None})
    members.update(same("end_heur", "end_flags") if want_goal_rows else {"end_heur": None, "end_flags": None})
    down = {"status": (u8, (3,)), "steps": (i32, (3,)), "cost": (f64, (3,)), "prefix_cost": (f64, (3,))}
    if want_end:
        down.update({"end_state": (f64, (4 * dim + 2, 3)), "end_hash": (u64, (3,))})
    if want_goal_rows:
        down.update({"end_heur": (f64, (3,)), "end_flags": (u8, (3,))})
    check(monkeypatch, "Rollouts", dim, (N,), dict(want_end=want_end, want_goal_rows=want_goal_rows), nbytes, members,
          {"end_stride": 3}, down)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("cell_cap", [CELL_CAP, 0])
@pytest.mark.parametrize("want_counts", [True, False])
def test_rays(monkeypatch, dim, cell_cap, want_counts):
    nbytes = {"status": 3, "n_cells": 12 if want_counts else None, "first_hit": 12 if want_counts else None,
              "cells": 60 if cell_cap else None}  # [3][5] int32
    members = same("status")
    members.update(same("n_cells", "first_hit") if want_counts else {"n_cells": None, "first_hit": None})
    members.update(same("cells") if cell_cap else {"cells": None})
    down = {"status": (u8, (3,))}
    if want_counts:
        down.update({"n_cells": (i32, (3,)), "first_hit": (i32, (3,))})
    if cell_cap:
        down["cells"] = (i32, (3, 5))
    check(monkeypatch, "Rays", dim, (N,), dict(cell_cap=cell_cap, want_counts=want_counts), nbytes, members, {"cell_cap": cell_cap}, down)


@pytest.mark.parametrize("dim,seg_bytes", [(2, 720), (3, 1008)])  # [4D+2][horizon + 1][3] float64
@pytest.mark.parametrize("want_states", [True, False])
def test_traj_info(monkeypatch, dim, seg_bytes, want_states):
    nbytes = {"status": 3, "n_segs": 12, "total_time": 24, "effort": 120, "seg_state": seg_bytes if want_states else None}
    members = same("status", "n_segs", "total_time", "effort")
    members.update(same("seg_state") if want_states else {"seg_state": None})
    down = {"status": (u8, (3,)), "n_segs": (i32, (3,)), "total_time": (f64, (3,)), "effort": (f64, (5, 3))}
    if want_states:
        down["seg_state"] = (f64, (4 * dim + 2, 3, 3))
    check(monkeypatch, "TrajInfo", dim, (N, HORIZON), dict(want_states=want_states), nbytes, members,
          {"effort_stride": 3, "seg_stride": 3}, down)


@pytest.mark.parametrize("dim,rows", [(2, 11), (3, 15)])  # 4D+3 rows
@pytest.mark.parametrize("strides", [None, (4, 3)])
def test_traj_samples(monkeypatch, dim, rows, strides):
    ns, ss = (3, 2) if strides is None else strides
    out_bytes = {(11, 3): 528, (11, 4): 1056, (15, 3): 720, (15, 4): 1440}[(rows, ns)]  # [rows][n_stride][sample_stride] float64
    kw = {} if strides is None else dict(n_stride=4, sample_stride=3)
    check(monkeypatch, "TrajSamples", dim, (N, COUNT), kw, {"out": out_bytes, "status": 3},
          {"out": ("out", "samples"), "status": ("status", "status")}, {"row_stride": 6 if strides is None else 12, "sample_stride": ss},
          {"samples": (f64, (rows, ns, ss)), "status": (u8, (3,))})


@pytest.mark.parametrize("dim", [2, 3])
def test_traj_traverse(monkeypatch, dim):
    check(monkeypatch, "TrajTraverse", dim, (N,), {}, {"status": 3, "cost": 24, "n_samples": 12, "n_cells": 12, "stop_sample": 12},
          same("status", "cost", "n_samples", "n_cells", "stop_sample"), {},
          {"status": (u8, (3,)), "cost": (f64, (3,)), "n_samples": (i32, (3,)), "n_cells": (i32, (3,)), "stop_sample": (i32, (3,))})


# coeff: [w_max - 1][2 (so + 1)][D][3] float64
@pytest.mark.parametrize("dim,so,coeff_bytes", [(2, 0, 288), (2, 1, 576), (2, 2, 864), (3, 0, 432), (3, 1, 864), (3, 2, 1296)])
def test_solve_out(monkeypatch, dim, so, coeff_bytes):
    members = same("status", "n_segs", "total_time", "coeff", "yaw_coeff", "taus")
    members["dts_out"] = ("dts", "dts")
    check(monkeypatch, "SolveOut", dim, (N, W_MAX, so), {},
          {"status": 3, "n_segs": 12, "total_time": 24, "coeff": coeff_bytes, "dts": 72, "yaw_coeff": 144, "taus": 96}, members,
          {"coeff_stride": 3, "dts_out_stride": 3, "yaw_stride": 3, "taus_stride": 3},
          {"status": (u8, (3,)), "n_segs": (i32, (3,)), "total_time": (f64, (3,)), "coeff": (f64, (3, 2 * (so + 1), dim, 3)),
           "dts": (f64, (3, 3)), "yaw_coeff": (f64, (3, 2, 3)), "taus": (f64, (4, 3))})


@pytest.mark.parametrize("dim", [2, 3])
def test_load_out(monkeypatch, dim):
    check(monkeypatch, "LoadOut", dim, (N, W_MAX), {}, {"status": 3, "n_segs": 12, "total_time": 24, "taus": 96},
          same("status", "n_segs", "total_time", "taus"), {"taus_stride": 3},
          {"status": (u8, (3,)), "n_segs": (i32, (3,)), "total_time": (f64, (3,)), "taus": (f64, (4, 3))})


@pytest.mark.parametrize("dim,max_bytes", [(2, 48), (3, 72)])  # [D][3] float64
def test_poly_limits(monkeypatch, dim, max_bytes):
    check(monkeypatch, "PolyLimits", dim, (N,), {},
          {"max_vel": max_bytes, "max_acc": max_bytes, "max_jrk": max_bytes, "exceed": 3, "valid": 3, "first_bad": 12},
          same("max_vel", "max_acc", "max_jrk", "exceed", "valid", "first_bad"), {"max_stride": 3},
          {"max_vel": (f64, (dim, 3)), "max_acc": (f64, (dim, 3)), "max_jrk": (f64, (dim, 3)), "exceed": (u8, (3,)),
           "valid": (u8, (3,)), "first_bad": (i32, (3,))})


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("count", [COUNT, 0])
def test_lambda_rows(monkeypatch, dim, count):
    # Ts [w_max][3], segs [8][8][3]; tau rows [3][count], one element at least
    nbytes = {"status": 3, "scaled": 3, "n_lseg": 12, "total": 24, "max_l": 24, "t_lo": 24, "t_hi": 24, "Ts": 96, "segs": 1536,
              "tau": 48 if count else 8, "lam": 48 if count else 8, "lam_dot": 48 if count else 8, "found": 6 if count else 1}
    down = {"status": (u8, (3,)), "n_lseg": (i32, (3,)), "total": (f64, (3,)), "Ts": (f64, (4, 3)), "segs": (f64, (8, 8, 3)),
            "scaled": (u8, (3,)), "max_l": (f64, (3,)), "t_lo": (f64, (3,)), "t_hi": (f64, (3,))}
    if count:
        down.update({"tau": (f64, (3, 2)), "lambda": (f64, (3, 2)), "lambda_dot": (f64, (3, 2)), "found": (u8, (3, 2))})
    lam = same("status", "n_lseg", "total", "Ts", "segs")
    check(monkeypatch, "LambdaRows", dim, (N, W_MAX), dict(count=count), nbytes, lam, {"ts_stride": 3, "seg_stride": 3}, down)
    # mplx_scale_down_out: its own four rows and the mplx_lambda_out inside it
    check(monkeypatch, "LambdaRows", dim, (N, W_MAX), dict(count=count), nbytes, same("scaled", "max_l", "t_lo", "t_hi"), {}, down,
          struct=lambda o: o.c_down(), host=False)
    check(monkeypatch, "LambdaRows", dim, (N, W_MAX), dict(count=count), nbytes, lam, {"ts_stride": 3, "seg_stride": 3}, down,
          struct=lambda o: o.c_down().lam, host=False)
    # mplx_tau_out
    check(monkeypatch, "LambdaRows", dim, (N, W_MAX), dict(count=count), nbytes,
          {"tau": ("tau", "tau"), "lam": ("lam", "lambda"), "lam_dot": ("lam_dot", "lambda_dot"), "found": ("found", "found")},
          {"stride": count}, down, struct=lambda o: o.c_tau(), host=False)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("want_pairs", [True, False])
def test_conflicts(monkeypatch, dim, want_pairs):
    nbytes = {"first_step": 12, "first_partner": 12, "min_d2": 24, "status": 3, "pair_first": 36 if want_pairs else None}  # [3][3] int32
    members = same("first_step", "first_partner", "min_d2", "status")
    members.update(same("pair_first") if want_pairs else {"pair_first": None})
    down = {"first_step": (i32, (3,)), "first_partner": (i32, (3,)), "min_d2": (f64, (3,)), "status": (u8, (3,))}
    if want_pairs:
        down["pair_first"] = (i32, (3, 3))
    check(monkeypatch, "Conflicts", dim, (N,), dict(want_pairs=want_pairs), nbytes, members, {"pair_stride": 3 if want_pairs else 0}, down)
    obj = E.Conflicts(FakeEnv(dim), N, want_pairs)
    assert len(obj._all()) == (5 if want_pairs else 4)


def test_empty_sets_keep_one_element(monkeypatch):
    """n = 0: every buffer still holds one element (a null pointer would read as `row not wanted`)."""
    monkeypatch.setattr(sys.modules[E.Rollouts.__module__], "DeviceArray", FakeArray)
    env = FakeEnv(2)
    r = E.Rollouts(env, 0, want_end=True, want_goal_rows=True)
    assert [getattr(r, k).nbytes for k in ("status", "steps", "cost", "prefix_cost", "end_state", "end_hash", "end_heur", "end_flags")] == \
        [1, 4, 8, 8, 80, 8, 8, 1]
    c = E.Conflicts(env, 0, want_pairs=True)
    assert [b.nbytes for b in c._all()] == [4, 4, 8, 1, 4]
    t = E.TrajSamples(env, 0, 0)
    assert (t.out.nbytes, t.status.nbytes) == (8, 1)
    assert r.download()["end_state"].shape == (10, 0) and c.download()["pair_first"].shape == (0, 0)
