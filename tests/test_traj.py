"""Trajectory<Dim> on the device (include/mplx_traj.h, csrc/traj_kernel.hip), CPU side: the numpy model
(tests/traj_model.py) against the committed fixture the reference's own Trajectory and env_map::traverse_trajectory
wrote (tests/golden/make_traj_golden.py), bit pattern for bit pattern; the terminal classes of the traversal the fixture
holds; the known-answer corridor plan; the header, the library's exports and the bindings."""
import ctypes as C
import os

import numpy as np
import pytest

import traj_model as M
from test_map_util import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "traj_golden.npz")

_CACHE = {}


def fixture():
    """[(case, trajs, queries)] and the loaded .npz, once per session."""
    if not _CACHE:
        cases = []
        for case in M.fixture_cases():
            trajs = M.case_trajs(case)
            cases.append((case, trajs, M.fixture_queries(case, trajs)))
        _CACHE["cases"], _CACHE["z"] = cases, np.load(GOLDEN)
    return _CACHE["cases"], _CACHE["z"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def model_traverse(case, trajs, mode):
    md, org, res = case["geo"]
    _, with_pot, grad_w = mode
    return M.traverse_set(trajs, case["grid"], case["pot"] if with_pot else None, md, org, res, case["v_max"], M.POT_W, grad_w)


def test_fixture_holds_what_the_issue_lists():
    cases, z = fixture()
    assert os.path.getsize(GOLDEN) <= 500 * 1024
    names = [c[0]["name"] for c in cases]
    assert len(names) == 8 * 2 * 2 + 3 and len(set(names)) == len(names)
    assert {(c[0]["control"], c[0]["dim"], c[0]["dt"]) for c in cases[:32]} == {(c, d, dt) for c in M.CONTROLS for d in (2, 3)
                                                                                 for dt in (0.7, 1.0)}
    for case, trajs, _ in cases[:32]:
        assert sorted(t.S for t in trajs) == [0, 1, 2, 3, 4, 5]
        md, org, res = case["geo"]
        assert (md, org, res) == (M.MAP2 if case["dim"] == 2 else M.MAP3) and len(set(md)) == len(md) and all(o != 0 for o in org)
        assert set(np.unique(case["pot"]).tolist()) >= {-1, 0, 1, 99, 100}


def test_model_equals_the_reference_on_every_bit_pattern():
    cases, z = fixture()
    for case, trajs, queries in cases:
        name = case["name"]
        head = z[name + "/head"].view(np.float64)
        for k, tr in enumerate(trajs):
            what = (name, k)
            assert head[k, 0] == tr.S, what
            assert bits(head[k, 1]) == bits(tr.T), what
            if tr.S == 0:  # (the reference's J over no segment: 0)
                assert not head[k, 2:].any() and not tr.effort.any()
                continue
            assert np.array_equal(bits(head[k, 2:7]), bits(tr.effort)), (what, head[k, 2:7], tr.effort)
            assert np.array_equal(z[name + "/cmd_u"][k].T, bits(tr.sample(M.UNIFORM_N, M.COMMAND))), what
            assert np.array_equal(z[name + "/way_u"][k].T, bits(tr.sample(M.UNIFORM_N, M.WAYPOINT))), what
            assert np.array_equal(z[name + "/cmd_q"][k].T, bits(tr.evaluate(queries[k], M.COMMAND))), what
            assert np.array_equal(z[name + "/way_q"][k].T, bits(tr.evaluate(queries[k], M.WAYPOINT))), what
        trav = z[name + "/trav"].view(np.float64)
        for m, mode in enumerate(M.MODES):
            r = model_traverse(case, trajs, mode)
            live = np.array([t.S > 0 for t in trajs])
            assert np.array_equal(bits(trav[live, m, 0]), bits(r["cost"][live])), (name, mode[0], trav[:, m, 0], r["cost"])
            assert np.array_equal(trav[live, m, 1].astype(np.int32), r["n_samples"][live]), (name, mode[0])
            assert (r["cost"][~live] == 0.0).all() and (r["status"][~live] & M.EMPTY).all()


def test_every_terminal_class_of_traverse_is_in_the_fixture():
    cases, z = fixture()
    seen = {k: 0 for k in ("zero", "finite positive", "inf by occupied cell", "inf by outside", "inf by potential >= 100",
                           "alias skip", "empty", "skipped samples")}
    for case, trajs, _ in cases:
        md, org, res = case["geo"]
        for mode in M.MODES:
            r = model_traverse(case, trajs, mode)
            for k, tr in enumerate(trajs):
                cost, stop = r["cost"][k], int(r["stop_sample"][k])
                if tr.S == 0:
                    seen["empty"] += 1
                    continue
                seen["skipped samples"] += int(r["n_cells"][k] < r["n_samples"][k])
                if cost == 0.0:
                    seen["zero"] += 1
                elif np.isfinite(cost):
                    assert cost > 0
                    seen["finite positive"] += 1
                else:
                    rows = tr.sample(int(r["n_samples"][k]) - 1)
                    idx, outside = M.cell_index(rows[:tr.dim, stop:stop + 1], md, org, res)
                    if outside[0]:
                        seen["inf by outside"] += 1
                    elif mode[1]:
                        assert case["pot"][idx[0]] >= 100
                        seen["inf by potential >= 100"] += 1
                    else:
                        assert case["grid"][idx[0]] == 100
                        seen["inf by occupied cell"] += 1
                # an outside sample the skip swallowed: its index equals the previous sample's
                rows = tr.sample(int(r["n_samples"][k]) - 1)
                idx, outside = M.cell_index(rows[:tr.dim], md, org, res)
                last = len(idx) if stop < 0 else max(stop, 1)
                seen["alias skip"] += int((outside[1:last] & (idx[1:last] == idx[:last - 1]) & ~outside[:last - 1]).any())
    assert all(v >= 1 for v in seen.values()), seen
    assert min(seen["zero"], seen["finite positive"], seen["inf by occupied cell"], seen["inf by outside"],
               seen["inf by potential >= 100"]) >= 10, seen


def test_hand_cases_against_the_reference():
    cases, z = fixture()
    by = {c[0]["name"]: c for c in cases}
    # the index alias: an outside cell with the index of the previous in-map cell is skipped, the reference returns 0
    case, trajs, _ = by["hand_alias"]
    md, org, res = case["geo"]
    rows = trajs[0].sample(1)
    idx, outside = M.cell_index(rows[:2], md, org, res)
    assert idx.tolist() == [24, 24] and outside.tolist() == [False, True]
    assert z["hand_alias/trav"].view(np.float64)[0, :, 0].tolist() == [0.0, 0.0, 0.0]
    r = model_traverse(case, trajs, M.MODES[0])
    assert (r["cost"][0], r["n_samples"][0], r["n_cells"][0], r["stop_sample"][0]) == (0.0, 2, 1, -1)
    # the boundary pair: at t = taus[1] the Command is still on segment 0, the Waypoint on segment 1
    case, trajs, queries = by["hand_boundary"]
    q = int(np.nonzero(queries[0] == 1.0)[0][0])
    assert z["hand_boundary/cmd_q"].view(np.float64)[0, q, 4] == 0.5 and z["hand_boundary/way_q"].view(np.float64)[0, q, 4] == -0.5
    assert trajs[0].evaluate([1.0], M.COMMAND)[4, 0] == 0.5 and trajs[0].evaluate([1.0], M.WAYPOINT)[4, 0] == -0.5
    # taus by sequential addition: the reference's T of 4 x 0.7 (and 3 x 0.7 is not 2.1)
    case, trajs, queries = by["hand_4x07"]
    T = z["hand_4x07/head"].view(np.float64)[0, 1]
    assert bits(T) == bits(0.7 + (0.7 + (0.7 + (0.7 + 0.0)))) == bits(trajs[0].T)
    assert trajs[0].taus[3] == 2.0999999999999996 != 2.1
    # times below 0 and above T clamp; the t row keeps the caller's time
    assert (queries[0] < 0).any() and (queries[0] > trajs[0].T).any()
    rows = trajs[0].evaluate(queries[0], M.COMMAND)
    assert np.array_equal(rows[10], queries[0])
    lo, hi = trajs[0].evaluate([0.0], M.COMMAND), trajs[0].evaluate([trajs[0].T], M.COMMAND)
    assert np.array_equal(rows[:10, queries[0] < 0], np.repeat(lo[:10], int((queries[0] < 0).sum()), axis=1))
    assert np.array_equal(rows[:10, queries[0] > trajs[0].T], np.repeat(hi[:10], int((queries[0] > trajs[0].T).sum()), axis=1))
    assert np.isnan(trajs[0].evaluate([np.nan, np.inf], M.WAYPOINT)).all()


def test_bad_action_and_bad_trajectories_in_the_model():
    U = M.control_table(0x03, 2)
    tr = M.Traj(0x03, 2, 1.0, U, np.zeros(10), [0, 1, len(U), 2])
    assert (tr.S, tr.status, tr.T) == (2, M.BAD_ACTION, 2.0)
    tr = M.Traj(0x03, 2, 1.0, U, np.zeros(10), [-2, 1])
    assert (tr.S, tr.status) == (0, M.BAD_ACTION | M.EMPTY)
    tr = M.Traj(0x03, 2, 1.0, U, np.zeros(10), [0])
    r = M.traverse(tr, np.zeros(64, np.int8), None, [8, 8], [-4.0, -4.0], 1e-300, 1e10, 0.1, 0.0)
    assert r["status"] == M.BAD and np.isnan(r["cost"]) and r["n_samples"] == 0


def test_corridor_plan_known_answer_through_the_model(engine):
    from test_plan_known_answer import corridor, run_c1
    ok, s, traj, _ = run_c1(engine)
    assert ok and s["segments"] == 35
    U = engine.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    tr = M.Traj(engine.ACC, 2, 1.0, U, traj.nodes[0], traj.actions)
    assert tr.S == 35 and tr.T == 35.0
    assert tr.effort.tolist() == [36.75, 1.5, 0.0, 0.0, 0.0]
    assert tr.effort[:4].tolist() == [traj.J(c) for c in (engine.VEL, engine.ACC, engine.JRK, engine.SNP)]
    c = corridor()
    r = M.traverse(tr, c["cells"], None, c["dim"], c["origin"], c["res"], 1.0, 0.1, 0.0)
    assert r["cost"] == 0.0 and r["stop_sample"] == -1 and r["n_samples"] == 701
    rows = tr.sample(35)
    assert np.array_equal(rows[:2].T, traj.getWaypoints()[:, :2])
    # (pos and vel: the rows an ACC primitive reads; a node the search reached twice keeps the acc of its first parent)
    assert np.array_equal(np.stack(tr.states)[:, :4], traj.getWaypoints()[:, :4])
    # the Python Trajectory without an engine env refuses instead of computing on the host
    with pytest.raises(RuntimeError):
        traj.sample(35)
    assert traj.getTotalTime() == 35.0


def test_traj_header_exports_and_bindings_agree(engine):
    calls = sorted(["mplx_traj_info_device", "mplx_traj_info", "mplx_traj_sample_device", "mplx_traj_sample",
                    "mplx_traj_traverse_device", "mplx_traj_traverse"])
    assert _declared("mplx_traj.h") == calls
    assert sorted(engine._abi.TRAJ_SYMBOLS) == calls
    others = engine._abi.SYMBOLS + engine._abi.MAP_UTIL_SYMBOLS + engine._abi.ROLLOUT_SYMBOLS + engine._abi.RAY_SYMBOLS
    assert not set(calls) & set(others)
    lib = C.CDLL(engine._abi.LIB_PATH)
    for s in calls:
        assert hasattr(lib, s), "libmplx.so does not export %s" % s
    L = engine._abi.lib()
    assert all(hasattr(L, s) for s in calls)
    assert L.mplx_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "mplx_traj.h")).read()
    assert "MPLX_TRAJ_EMPTY = 1, MPLX_TRAJ_BAD_ACTION = 2, MPLX_TRAJ_BAD = 4" in text
    assert "MPLX_TRAJ_COMMAND = 0, MPLX_TRAJ_WAYPOINT = 1" in text
    assert (engine.TRAJ_EMPTY, engine.TRAJ_BAD_ACTION, engine.TRAJ_BAD) == (M.EMPTY, M.BAD_ACTION, M.BAD)
    assert (engine.TRAJ_COMMAND, engine.TRAJ_WAYPOINT) == (M.COMMAND, M.WAYPOINT)
    # a NULL context is an argument error in every call, before anything else is looked at
    s, io = engine._abi.TrajSet(), engine._abi.TrajInfoOut()
    t, so, to = engine._abi.TrajTimes(), engine._abi.TrajSampleOut(), engine._abi.TrajTraverseOut()
    for suffix in ("_device", ""):
        assert getattr(L, "mplx_traj_info" + suffix)(None, C.byref(s), C.byref(io)) == engine._abi.ERR_ARG
        assert getattr(L, "mplx_traj_sample" + suffix)(None, C.byref(s), C.byref(t), C.byref(so)) == engine._abi.ERR_ARG
        assert getattr(L, "mplx_traj_traverse" + suffix)(None, C.byref(s), 0, C.byref(to)) == engine._abi.ERR_ARG
    # the struct layouts of the bindings are the header's (LP64: pointers and int64 8 bytes, int32 padded)
    assert (C.sizeof(engine._abi.TrajSet), C.sizeof(engine._abi.TrajInfoOut), C.sizeof(engine._abi.TrajTimes),
            C.sizeof(engine._abi.TrajSampleOut), C.sizeof(engine._abi.TrajTraverseOut)) == (56, 56, 32, 32, 40)
