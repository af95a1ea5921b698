"""MapUtil<Dim>::rayTrace and the ray trace of env_map::is_goal (include/mplx_ray.h, csrc/ray_kernel.hip), CPU side:
the numpy restatement (tests/ray_model.py) against the committed fixture made by the reference's own MapUtil and
env_map (tests/golden/make_ray_golden.py) and against the oracle's search region; the inputs of the GPU tests
(tests/test_gpu_ray.py) hold the classes they are meant to hold; the header and the library's exports; no CPU
fallback."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_model as R
from test_map_util import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ray_golden.npz")

_MODEL = {}


def fixture_model(case):
    """(p1, p2, model result) of a fixture case, computed once per session."""
    if case[0] not in _MODEL:
        p1, p2 = R.fixture_rays(case)
        _MODEL[case[0]] = (p1, p2, R.ray_trace(case[2], case[3], case[4], case[5], p1, p2))
    return _MODEL[case[0]]


def test_model_matches_the_golden_fixture_on_every_ray():
    """tests/golden/ray_golden.npz holds what the reference's rayTrace and is_goal returned: list lengths, every cell of
    every list in order, the first occupied cell, is_goal with the goal at p2."""
    z = np.load(GOLDEN)
    for case in R.fixture_cases():
        name = case[0]
        p1, p2, m = fixture_model(case)
        assert len(p1) == 4000
        assert np.array_equal(m["n_cells"], z[name + "/n_cells"]), name
        assert np.array_equal(m["cells"], np.cumsum(z[name + "/cell_steps"].astype(np.int64)).astype(np.int32)), name
        assert np.array_equal(m["first_hit"], z[name + "/first_hit"]), name
        goal, _ = R.is_goal(m, p1, p2, R.TOL_POS)
        assert np.array_equal(goal.astype(np.uint8), z[name + "/is_goal"]), name
        assert not (m["status"] & R.BAD).any()


def test_fixture_rays_hold_every_class():
    maps = R.fixture_cases()
    assert [c[3] for c in maps] == [[96, 89], [40, 33, 37], [65, 31]] and maps[2][5] == 0.05
    for case in maps:
        p1, p2, m = fixture_model(case)
        goal, inside = R.is_goal(m, p1, p2, R.TOL_POS)
        shares = {"hit": ((m["status"] & R.HIT) > 0).mean(), "left": ((m["status"] & R.LEFT_MAP) > 0).mean(),
                  "empty": (m["n_cells"] == 0).mean(), "inside but blocked": (inside & ~goal).mean()}
        assert all(v >= 0.02 for v in shares.values()), (case[0], shares)
        assert m["n_cells"].max() >= 40
        assert (p1[::97] == p2[::97]).all() and (m["n_cells"][::97] == 0).all()
        assert {-1, 0, 100, 101, 127, -5} <= set(np.unique(case[2]).tolist())  # and values in 1 .. 99
        assert ((case[2] > 0) & (case[2] < 100)).any()


def test_cell_sets_equal_the_oracles_search_region(oracle_lib):
    """MapPlanner::setSearchRegion with radius 0 marks the cells of rayTrace(p1, p2) and p2's cell: a second pin of the
    model that needs no new reference build (the reference's own MapPlanner where oracle/_ref exists)."""
    ref = os.path.exists(oracle_lib.REF_PLANNER_SO)
    for case in R.fixture_cases():
        name, dim, grid, md, org, res = case
        p1, p2, m = fixture_model(case)
        for k in range(0, 4000, 13):
            want = np.zeros(grid.size, np.uint8)
            want[m["cells"][m["offs"][k]:m["offs"][k + 1]]] = 1
            c = R.c_round((p2[k] - np.asarray(org)) / res - 0.5)
            if ((c >= 0) & (c < np.asarray(md))).all():
                want[int(sum(int(c[i]) * int(np.prod(md[:i])) for i in range(dim)))] = 1
            got = oracle_lib.search_region(md, org, res, np.stack([p1[k], p2[k]]), [0.0] * dim, ref=ref)
            assert np.array_equal(got != 0, want != 0), (name, k)


def test_hand_cases():
    md, org, res = [12, 5], [0.0, 0.0], 0.1
    grid = np.zeros(60, np.int8)
    grid[2 * 12 + 4] = 100
    y = 0.25

    def one(a, b):
        m = R.ray_trace(grid, md, org, res, np.array([a]), np.array([b]))
        return int(m["max_diff"][0]), m["cells"].tolist(), int(m["status"][0]), int(m["first_hit"][0])

    assert one([0.25, y], [0.25, y]) == (0, [], 0, -1)                     # max_diff 0
    assert one([0.25, y], [0.35, y])[:2] == (1, [])                        # 1: no step
    assert one([0.25, y], [0.45, y])[:2] == (2, [24 + 3])                  # 2: the one step in between
    # an axis ray of exactly 5 cells: cells 1 .. 5 of row 2, neither end cell (0 and 6); cell 4 is occupied
    md5, cells, status, hit = one([0.05, y], [0.65, y])
    assert (md5, cells, status, hit) == (7, [25, 26, 27, 28, 29], R.HIT, 28)
    # leaves at its first step
    assert one([-0.35, y], [0.65, y]) == (12, [], R.LEFT_MAP, -1)
    # values that are not occupied (map_util.h:48), and BAD rays
    for v in (37, 101, 127, -5, -1):
        grid[2 * 12 + 4] = v
        assert one([0.05, y], [0.65, y])[2:] == (0, -1)
    for bad in ([np.nan, y], [np.inf, y], [1e300, y]):
        assert one(bad, [0.65, y]) == (0, [], R.BAD, -1)
    out, status = R.cells_matrix(R.ray_trace(grid, md, org, res, np.array([[0.05, y]]), np.array([[0.65, y]])), 3, -7)
    assert out.tolist() == [[25, 26, 27]] and status.tolist() == [R.TRUNCATED]


def test_ray_header_declares_the_three_calls_and_the_library_exports_them(engine):
    calls = sorted(["mplx_ray_trace_device", "mplx_ray_trace", "mplx_goal_sight_device"])
    assert _declared("mplx_ray.h") == calls
    assert sorted(engine._abi.RAY_SYMBOLS) == calls
    assert not set(calls) & set(engine._abi.SYMBOLS)  # mplx.h keeps its ABI version
    assert not set(calls) & set(engine._abi.MAP_UTIL_SYMBOLS + engine._abi.ROLLOUT_SYMBOLS)
    lib = C.CDLL(engine._abi.LIB_PATH)
    for s in calls:
        assert hasattr(lib, s), "libmplx.so does not export %s" % s
    L = engine._abi.lib()
    assert all(hasattr(L, s) for s in calls)
    text = open(os.path.join(ROOT, "include", "mplx_ray.h")).read()
    assert "MPLX_RAY_LEFT_MAP = 1, MPLX_RAY_HIT = 2, MPLX_RAY_BAD = 4, MPLX_RAY_TRUNCATED = 8" in text
    assert "MPLX_FLAG_GOAL_BLOCKED = 8" in text
    assert (engine.RAY_LEFT_MAP, engine.RAY_HIT, engine.RAY_BAD, engine.RAY_TRUNCATED) == (R.LEFT_MAP, R.HIT, R.BAD, R.TRUNCATED)


def test_map_util_ray_trace_has_no_cpu_fallback(engine):
    import torch
    name, dim, grid, md, org, res = R.fixture_cases()[0]
    p1, p2, m = fixture_model(R.fixture_cases()[0])
    k = int(np.argmax(m["n_cells"]))
    mu = engine.MapUtil(dim)
    mu.setMap(org, md, grid, res)
    if torch.cuda.is_available():  # (the same call on a machine with a GPU: the device result)
        cells = mu.rayTrace(p1[k], p2[k])
        assert cells.dtype == np.int32 and cells.shape == (m["n_cells"][k], dim)
        assert np.array_equal(cells[:, 0] + md[0] * cells[:, 1], m["cells"][m["offs"][k]:m["offs"][k + 1]])
        mu.close() if hasattr(mu, "close") else None
        return
    with pytest.raises(engine._abi.MplxError) as e:
        mu.rayTrace(p1[k], p2[k])
    assert e.value.code == engine._abi.ERR_NO_DEVICE and "no CPU fallback" in str(e.value)


def test_round_boundary_set_holds_every_class():
    p1, p2, classes = R.boundary_set()
    assert len(classes) == 3 * 10 + 3
    for label, idx in classes.items():
        assert len(idx) >= 1, "no ray for: " + label
    assert len(p1) >= 33 and len(p1) == len(p2)
    g = R.boundary_map()
    assert (g == 100).sum() == 8 and (g == 0).sum() == g.size - 9
    # the classes are what they say: recomputed on the picked rays alone
    m = R.ray_trace(g, R.BOUNDARY_MD, R.BOUNDARY_ORG, R.BOUNDARY_RES, p1, p2)
    emitted, valid, out_step, hit_step = R.step_tables(m)
    for G in (4, 16, 64):
        for t in (G - 1, G, G + 1, 2 * G, 2 * G + 1):
            assert (m["max_diff"][classes["G%d: %d steps" % (G, t)]] - 1 == t).all()
        for k in classes["G%d: duplicate across a round boundary" % G]:
            assert any(valid[k] >= b + 1 and not emitted[k, b + 1] for b in (G, 2 * G, 3 * G) if b + 1 < emitted.shape[1])
        assert (out_step[classes["G%d: first outside step at kG" % G]] % G == 0).all()
        assert (out_step[classes["G%d: first outside step at kG+1" % G]] % G == 1).all()
        assert (hit_step[classes["G%d: first hit at kG" % G]] % G == 0).all()
        assert (hit_step[classes["G%d: first hit at kG+1" % G]] % G == 1).all()
    assert (hit_step[classes["first hit at step 1"]] == 1).all()
    k = classes["first hit at the last step"]
    assert (hit_step[k] == m["max_diff"][k] - 1).all()
    assert (out_step[classes["leaves at its first step"]] == 1).all()


@pytest.mark.parametrize("dim", [2, 3])
def test_goal_world_holds_blocked_and_clear_successors(engine, oracle_lib, dim):
    """Among the emitted successors of the goal world (the oracle's expansion), at least 30 are inside the goal
    tolerances (the oracle's goal_tol) with an occupied cell on the ray to the goal, and at least 30 with a clear one."""
    from helpers import oracle_env
    wl, goal, tol = R.goal_world(engine, dim)
    assert wl.map_dim == ([64, 61] if dim == 2 else [40, 37, 33])
    vals = np.unique(wl.grid).tolist()
    assert vals == [0, 37, 100, 101]
    dense = oracle_lib.expand(oracle_env(wl), wl.nodes, threads=4)
    emit = np.nonzero((dense["status"] == 1) | (dense["status"] == 2))[0]
    st = dense["state"][:, emit]
    in_tol, blocked = R.goal_world_model(wl, goal, tol, st[:dim])
    want = np.array([oracle_lib.goal_tol(dim, np.ascontiguousarray(st[:, k]), goal, tol) for k in range(emit.size)])
    assert np.array_equal(in_tol, want)
    assert blocked.sum() >= 30 and (in_tol & ~blocked).sum() >= 30, (int(blocked.sum()), int((in_tol & ~blocked).sum()))
