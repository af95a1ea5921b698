"""CPU: the semantics of include/mplx_table.h as tests/table_model.py restates them -- the label-correcting sweep reaches
the fixed point a heap Dijkstra reaches, and on the corridor of the reference's test_planner_2d it finds the cost the
reference publishes -- plus the plumbing of the new header (declared in _abi.py, parses as C).  Successors come from the
CPU oracle; no GPU."""
import math
import os
import re
import subprocess

import numpy as np

import large_case as LC
from helpers import oracle_env
from oracle import oracle as O
from table_model import TableArrays, TableModel, dijkstra, hand_case, hand_lists, oracle_provider, sweep
from test_gpu_parity import _small_world
from test_plan_known_answer import corridor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_start(wl):
    """A state at rest in a free cell near the middle of the workload's map."""
    md = wl.map_dim
    grid = np.asarray(wl.grid).reshape(md[::-1])
    free = np.argwhere(grid == 0)[:, ::-1]  # (x, y[, z])
    mid = np.array(md) / 2.0
    cell = free[np.argmin(np.abs(free - mid).sum(axis=1))]
    s = np.zeros(4 * wl.dim + 2)
    s[:wl.dim] = np.asarray(wl.origin) + (cell + 0.5) * wl.res
    return s


def test_sweep_reaches_the_fixed_point_of_dijkstra(engine):
    wl = _small_world(engine, 2, engine.ACC, seed=5, edge=32)
    oenv = oracle_env(wl)
    prov = oracle_provider(O, oenv)
    start = small_start(wl)
    h0 = O.lattice_hash(2, engine.ACC, start)
    model = TableModel(10)
    rounds, largest = sweep(model, prov, start, [h0])
    want = dijkstra(prov, start, h0)
    got = model.arrays()
    assert got["n_nodes"] > 200 and rounds > 3, (got["n_nodes"], rounds)  # a sweep worth the name
    reached = {int(h): float(g) for h, g in zip(got["hash"], got["g"]) if math.isfinite(g)}
    assert reached == want  # exact: both only add and compare doubles
    # nodes the sweep created but never reached: only blocked edges lead to them -- it has none (they do not count)
    assert len(reached) == got["n_nodes"]
    # every back-pointer is an edge of the final tree: g[v] = g[pred] + cost needs the lists, so check the order instead
    for i in range(1, got["n_nodes"]):
        assert got["pred"][i] >= 0 and got["g"][got["pred"][i]] < got["g"][i]
    assert got["pred"][0] == -1 and got["g"][0] == 0.0


def corridor_sweep_model(engine):
    c = corridor()
    U = engine.workloads.grid_controls([-0.5, 0.0, 0.5], 2)  # test_planner_2d.cpp:49-53
    oenv = O.Env(2, O.ACC, U, c["cells"], c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    start = engine.Waypoint(2, engine.ACC, pos=c["start"]).to_row()
    model = TableModel(10)
    rounds, largest = sweep(model, oracle_provider(O, oenv), start, [O.lattice_hash(2, O.ACC, start)], g_max=351.5)
    return c, model, rounds, largest


def test_corridor_sweep_finds_the_published_cost(engine):
    """reference README.md:199-202: T = 35, J(ACC) = 1.5 -> g = 10 * 35 + 1.5 = 351.5 (tests/test_plan_known_answer.py).
    A sweep bounded by that cost reaches the goal region in exactly one node, at exactly that cost."""
    c, model, rounds, largest = corridor_sweep_model(engine)
    got = model.arrays()
    near = np.nonzero(np.abs(got["state"][:2] - np.asarray(c["goal"])[:, None]).max(axis=0) <= 0.5)[0]
    assert near.size == 1 and got["g"][near[0]] == 351.5
    assert rounds == 36 and got["n_nodes"] == 21677
    assert model.counting - 1 == 114107 and largest == 1047  # (the seed is a counting entry too)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_models_agree(model, arr, got, want, what):
    """Everything a call returns and the full node arrays behind it, bit for bit: TableArrays against TableModel."""
    (got_fr, got_eid), (want_fr, want_eid) = got, want
    assert got_eid.dtype == want_eid.dtype and np.array_equal(got_eid, want_eid), what + ": entry ids"
    assert got_fr["count"] == want_fr["count"] and np.array_equal(got_fr["id"], want_fr["id"]), what + ": frontier ids / order"
    assert np.array_equal(_bits(got_fr["g"]), _bits(want_fr["g"])), what + ": frontier g"
    assert np.array_equal(_bits(got_fr["state"]), _bits(want_fr["state"])), what + ": frontier state rows"
    a, b = arr.arrays(), model.arrays()
    assert a["n_nodes"] == b["n_nodes"] and arr.counting == model.counting, what
    for k in ("hash", "pred", "pred_action"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), what + ": " + k
    for k in ("g", "state"):
        assert a[k].shape == b[k].shape and np.array_equal(_bits(a[k]), _bits(b[k])), what + ": " + k


def test_array_reference_is_the_model_on_the_hand_built_calls():
    """The three calls of tests/test_gpu_table.py::test_three_calls_on_one_table (new keys, equal, larger and smaller
    candidates, +inf and NaN costs, a parent without id, poisoned tails, the EMPTY hash, a cutting g_max) and the one call
    of test_one_relax_on_hand_built_lists, then seeds into the same table: TableArrays returns what TableModel returns."""
    rng, pool, host, parent_id, parent_g = hand_case(seed=12, n=120, S=40)
    model, arr = TableModel(10), TableArrays(10)
    other = lambda pid, by: np.where(pid < 0, -1, pid + by).astype(np.int32)
    host3 = hand_lists(rng, 120, 40, np.concatenate([pool, rng.integers(1, 2 ** 63, size=300, dtype=np.uint64)]), 0xBEEF00000000)
    pg3 = np.maximum(parent_g + rng.choice([-0.5, 0.0, 0.75], size=120), 0.0)
    calls = [(host, parent_id, parent_g, math.inf), (host, other(parent_id, 5000), parent_g, math.inf),
             (host3, other(parent_id, 9000), pg3, 4.0)]
    counts = []
    for k, (lists, pid, pg, g_max) in enumerate(calls):
        got, want = arr.relax(lists, pid, pg, g_max), model.relax(lists, pid, pg, g_max)
        assert_models_agree(model, arr, got, want, "call %d" % (k + 1))
        counts.append(want[0]["count"])
    assert counts[0] > 500 and counts[1] == 0 and counts[2] > 100 and model.n_nodes > 1500
    cut = host3["cost"] + np.repeat(pg3, 40)
    assert (cut[np.isfinite(cut)] > 4.0).sum() > 100  # g_max did cut
    # a shorter n_nodes, and seeds: known and new hashes, g from a list with values that do not count
    args = (host3, parent_id, parent_g * 0.5, 3.25)
    got, want = arr.relax(*args, n_nodes=77), model.relax(*args, n_nodes=77)
    assert_models_agree(model, arr, got, want, "n_nodes = 77")
    states = rng.standard_normal((10, 9))
    hashes = np.array([model.hash[3], 7, 7, 8, model.hash[0], 9, 10, 11, 8], dtype=np.uint64)
    g = np.array([0.0, 0.5, 0.25, np.nan, -0.0, np.inf, -1.0, 0.0, 1.0])
    assert_models_agree(model, arr, arr.seed(states, hashes, g), model.seed(states, hashes, g), "seed")
    assert_models_agree(model, arr, arr.seed(states[:, 0], hashes[:1]), model.seed(states[:, 0], hashes[:1]), "one seed")
    # the first call of the 300 x 40 case on fresh tables
    rng, pool, host, parent_id, parent_g = hand_case()
    model, arr = TableModel(10), TableArrays(10)
    args = (host, parent_id, parent_g, 3.25)
    assert_models_agree(model, arr, arr.relax(*args), model.relax(*args), "300 x 40")


def test_the_large_scenario_covers_what_it_claims():
    """tests/large_case.py on the array reference alone: what keeps tests/test_gpu_table_large.py from being vacuous
    (the GPU tests repeat it).  The reference follows 9.3 M entries, once per process."""
    sc, snaps = LC.reference(O.lattice_hash(2, O.ACC, LC.goal_row()))
    LC.assert_table_conditions(sc, snaps)


def _declared(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))


def test_every_function_of_the_header_is_declared_in_abi(engine):
    syms = _declared("mplx_table.h")
    assert "mplx_table_relax_device" in syms and "mplx_table_seed" in syms and "mplx_table_path" in syms
    assert sorted(engine._abi.TABLE_SYMBOLS) == syms
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s
    import ctypes as C
    assert C.sizeof(engine._abi.TableView) == 6 * 8 and C.sizeof(engine._abi.TableFrontier) == 6 * 8


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_table.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
