"""CPU: the semantics of include/mplx_open.h as tests/open_model.py restates them -- on the corridor of the reference's
test_planner_2d the batched rule finds the published cost 351.5 without a bound known in advance, with a tenth of the
expansions of the bounded sweep -- plus the plumbing of the new header (declared in _abi.py, parses as C).  Successors
come from the CPU oracle; no GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import large_case as LC
import open_model as OM
from oracle import oracle as O
from table_model import TableArrays, TableModel, oracle_provider
from test_plan_known_answer import corridor
from test_table import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP_NODES = 21677  # tests/test_table.py: the sweep bounded by g_max = 351.5 creates this many nodes (and expands them)


def corridor_setup(engine, cells=None, blocked=False):
    c = corridor()
    grid = np.array(c["cells"], dtype=np.int8) if cells is None else cells
    U = engine.workloads.grid_controls([-0.5, 0.0, 0.5], 2)  # test_planner_2d.cpp:49-53
    oenv = O.Env(2, O.ACC, U, grid, c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    start = engine.Waypoint(2, engine.ACC, pos=c["start"]).to_row()
    goal = engine.Waypoint(2, engine.ACC, pos=c["goal"]).to_row()
    table = TableModel(10)
    ray = OM.ray_blocked(grid, c["dim"], c["origin"], c["res"], goal[:2]) if blocked else None
    opn = OM.OpenModel(table, 2, goal, O.lattice_hash(2, O.ACC, goal), w=10.0, v_max=1.0, tol_pos=0.5, blocked=ray)
    return c, table, opn, oracle_provider(O, oenv), start, O.lattice_hash(2, O.ACC, start)


def corridor_search(engine, eps, delta, capacity, sight=0, **kw):
    c, table, opn, prov, start, h0 = corridor_setup(engine, blocked=bool(sight))
    out = OM.search(table, opn, prov, start, h0, eps, delta, capacity, sight=sight, **kw)
    return table, opn, out


# (eps, delta, frontier capacity) -> rounds, expanded, nodes, truncated selections, goal_f (the goal node lies 0.5 m from
# the goal: h = w * 0.5 / v_max = 5, goal_f = 351.5 + 5 eps)
CORRIDOR = {
    (1.0, 0.0, 65536): (49, 586, 1780, 0, 356.5),
    (1.0, 2.0, 65536): (35, 1419, 3129, 0, 356.5),
    (1.0, 10.0, 64): (98, 6075, 10098, 91, 356.5),
    (2.0, 5.0, 65536): (35, 1390, 2957, 0, 361.5),
    (0.0, 10.0, 65536): (35, 21669, 22141, 0, 351.5),
}


@pytest.mark.parametrize("case", sorted(CORRIDOR))
def test_corridor_search_finds_the_published_cost(engine, case):
    """reference README.md:199-202: g = 10 * 35 + 1.5 = 351.5.  Every configuration ends FOUND at exactly that cost with
    exactly one goal-region node at goal_f; rounds (relax calls), expansions and nodes are pinned."""
    eps, delta, cap = case
    rounds, expanded, nodes, truncated, goal_f = CORRIDOR[case]
    table, opn, out = corridor_search(engine, eps, delta, cap)
    res = out["result"]
    print(case, out["rounds"], out["expanded"], table.n_nodes, out["truncated"], res)
    assert out["status"] == OM.FOUND and res["goal_g"] == 351.5 and res["goal_f"] == goal_f
    at_goal_f = [i for i, fl in opn.flags.items() if fl & OM.IS_GOAL and opn.f[i] == res["goal_f"]]
    assert at_goal_f == [res["goal_id"]]
    assert (out["rounds"], out["expanded"], out["truncated"]) == (rounds, expanded, truncated)
    assert table.n_nodes == nodes
    if case == (1.0, 0.0, 65536):
        assert out["expanded"] < SWEEP_NODES / 10  # the feature's point: goal-directed, and no bound known in advance
    # the chain of best predecessors: 35 edges back to the seed
    i, edges = res["goal_id"], 0
    while table.pred[i] >= 0:
        i, edges = table.pred[i], edges + 1
    assert i == 0 and edges == 35


def test_corridor_with_the_ray_trace_keeps_the_answer(engine):
    table, opn, out = corridor_search(engine, 1.0, 10.0, 65536, sight=1)
    assert out["status"] == OM.FOUND and out["result"]["goal_g"] == 351.5


def blocked_goal_cells():
    """The corridor with the goal's cell and every cell that touches its tolerance box occupied."""
    c = corridor()
    md = c["dim"]
    grid = np.array(c["cells"], dtype=np.int8).reshape(md[1], md[0]).copy()
    cell = np.floor((np.asarray(c["goal"]) - np.asarray(c["origin"])) / c["res"]).astype(int)
    r = int(math.ceil(0.5 / c["res"])) + 1
    grid[max(cell[1] - r, 0):cell[1] + r + 1, max(cell[0] - r, 0):cell[0] + r + 1] = 100
    return np.ascontiguousarray(grid.ravel())


def test_goal_in_an_occupied_cell_ends_empty(engine):
    """No state enters the goal region, and under a finite g_max the open set runs dry."""
    _, table, opn, prov, start, h0 = corridor_setup(engine, cells=blocked_goal_cells())
    out = OM.search(table, opn, prov, start, h0, 1.0, 10.0, 65536, g_max=60.0)
    res = out["result"]
    assert out["status"] == OM.EMPTY and res["goal_id"] == -1 and res["goal_f"] == math.inf and res["goal_g"] == math.inf
    assert res["f_min"] == math.inf and res["n_open"] == 0 and res["count"] == 0
    assert out["expanded"] > 50 and not any(fl & (OM.IS_OPEN | OM.IS_GOAL) for fl in opn.flags.values())


def test_limits_stop_early_and_reopen_the_selection(engine):
    table, opn, out = corridor_search(engine, 1.0, 10.0, 65536, max_rounds=5)
    assert out["status"] == OM.MAX_ROUNDS and out["rounds"] == 5
    n_open = sum(1 for fl in opn.flags.values() if fl & OM.IS_OPEN)
    assert n_open == out["result"]["n_open"] + out["result"]["count"] and out["result"]["count"] > 0
    table, opn, out = corridor_search(engine, 1.0, 10.0, 65536, max_expand=40)
    assert out["status"] == OM.MAX_EXPAND and 0 < out["expanded"] <= 40


def test_select_on_an_empty_open_set_is_empty_with_infinite_f_min():
    table = TableModel(10)
    opn = OM.OpenModel(table, 2, np.zeros(10), 1, 10.0, 1.0)
    res, fr = opn.select(0.0, 8)
    assert res == {"status": OM.EMPTY, "goal_id": -1, "count": 0, "n_open": 0, "f_min": math.inf, "goal_f": math.inf,
                   "goal_g": math.inf} and fr["count"] == 0


def hand_model(O_):
    """The hand-built scenario of the GPU test on the model alone: (table, open set, states, the scenario's parts)."""
    states, goal, in_goal, ignored, push1, push2 = OM.hand_scenario()
    hashes = [O_.lattice_hash(2, O_.ACC, states[:, k]) for k in range(OM.HAND_N)]
    table = TableModel(10)
    fr, _ = table.seed(states, hashes)
    assert fr["count"] == OM.HAND_N and table.n_nodes == OM.HAND_N  # distinct lattice states
    opn = OM.OpenModel(table, 2, goal, O_.lattice_hash(2, O_.ACC, goal), OM.HAND_W, OM.HAND_VMAX, tol_pos=OM.HAND_TOL)
    return table, opn, states, goal, in_goal, ignored, push1, push2


def test_the_hand_built_scenario_covers_what_it_claims():
    """Equal keys, truncated selections, every status, ignored rows, re-opened nodes, replaced keys and a tie among the
    goal nodes at FOUND: properties of the inputs of tests/test_gpu_open.py, checked where no GPU is needed."""
    table, opn, states, goal, in_goal, ignored, push1, push2 = hand_model(O)
    assert in_goal.sum() == 121
    opn.push(OM.hand_frontier(states, push1, with_tail=True), len(push1["id"]), 1.0)
    f, fl = opn.arrays()
    seen = (fl & OM.SEEN) > 0
    assert seen.sum() == 1500 and not seen[ignored].any() and not seen[push1["tail_id"]].any()
    assert np.unique(f[seen]).size < seen.sum() / 2  # equal keys are common
    closed = set()
    for delta, cap in OM.HAND_SELECTS:
        res, sel = opn.select(delta, cap)
        assert res["status"] == OM.SELECTED and res["count"] == sel["count"] <= cap
        if (delta, cap) in ((2.5, 16), (math.inf, 16)):  # truncated: more were selected than fit
            assert res["count"] == 16 and any(fl & OM.IS_OPEN and opn.f[i] <= res["f_min"] + delta for i, fl in opn.flags.items())
        closed.update(int(i) for i in sel["id"])
    before = dict(opn.f)
    was_open = {i for i, fl in opn.flags.items() if fl & OM.IS_OPEN}
    opn.push(OM.hand_frontier(states, push2, with_tail=True), 10 ** 9, 1.0, capacity=len(push2["id"]))
    b = set(int(i) for i in push2["id"])
    assert len(closed & b) > 20 and all(opn.flags[i] & OM.IS_OPEN for i in closed & b)  # re-opened
    assert sum(1 for i in was_open & b if opn.f[i] != before[i]) > 50  # open keys replaced
    assert not any(int(i) in opn.flags for i in push2["tail_id"])
    statuses = []
    for _ in range(200):
        res, sel = opn.select(2.5, 5000)
        statuses.append(res["status"])
        if res["status"] != OM.SELECTED:
            break
    assert statuses[-1] == OM.FOUND and 5 < len(statuses) < 60 and res["n_open"] > 0
    tied = [i for i, fl in opn.flags.items() if fl & OM.IS_GOAL and opn.f[i] == res["goal_f"]]
    assert len(tied) >= 2 and res["goal_id"] == min(tied) and res["goal_g"] == 0.0  # (the table's g: the seeds' 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_array_reference_is_the_model_on_the_hand_built_scenario():
    """The calls of tests/test_gpu_open.py::test_hand_built_push_and_select (push 1, every select of HAND_SELECTS, push 2,
    selects until FOUND, clear, eps = 0) through OpenModel and OpenArrays: f, the flags, every result field and every
    frontier row bit for bit."""
    table, model, states, goal, in_goal, ignored, push1, push2 = hand_model(O)
    tarr = TableArrays(10)
    tarr.seed(states, np.array(table.hash, dtype=np.uint64))
    arr = OM.OpenArrays(tarr, 2, goal, model.goal_hash, OM.HAND_W, OM.HAND_VMAX, tol_pos=OM.HAND_TOL)

    def same_open(what):
        (f, fl), (wf, wfl) = arr.arrays(), model.arrays()
        assert fl.dtype == wfl.dtype and np.array_equal(fl, wfl), what + ": flags"
        assert np.array_equal(_bits(f), _bits(wf)), what + ": f"

    def select_both(delta, cap, what):
        (got, got_fr), (want, want_fr) = arr.select(delta, cap), model.select(delta, cap)
        assert list(got) == list(want), what
        for k in want:
            same = type(got[k]) is type(want[k]) and _bits([got[k]])[0] == _bits([want[k]])[0]
            assert same, "%s: %s %r != %r" % (what, k, got[k], want[k])
        assert got_fr["count"] == want_fr["count"] and got_fr["id"].dtype == want_fr["id"].dtype, what
        assert np.array_equal(got_fr["id"], want_fr["id"]), what + ": frontier ids / order"
        assert np.array_equal(_bits(got_fr["g"]), _bits(want_fr["g"])), what + ": frontier g"
        assert got_fr["state"].shape == want_fr["state"].shape, what
        assert np.array_equal(_bits(got_fr["state"]), _bits(want_fr["state"])), what + ": frontier state rows"
        same_open(what)
        return want

    same_open("new")
    assert select_both(0.0, 8, "nothing pushed")["status"] == OM.EMPTY
    host = OM.hand_frontier(states, push1, with_tail=True)
    arr.push(host, len(push1["id"]), 1.0)
    model.push(host, len(push1["id"]), 1.0)
    same_open("push 1")
    for delta, cap in OM.HAND_SELECTS:
        assert select_both(delta, cap, "select(%r, %d)" % (delta, cap))["status"] == OM.SELECTED
    host = OM.hand_frontier(states, push2, with_tail=True)
    arr.push(host, 10 ** 9, 1.0, capacity=len(push2["id"]))
    model.push(host, 10 ** 9, 1.0, capacity=len(push2["id"]))
    same_open("push 2")
    for k in range(200):
        res = select_both(2.5, 5000, "select %d after push 2" % k)
        if res["status"] != OM.SELECTED:
            break
    assert res["status"] == OM.FOUND and k > 5
    arr.f[:], arr.flags[:] = 0.0, 0
    model.f, model.flags = {}, {}
    arr.push(host, 100, 0.0)
    model.push(host, 100, 0.0)
    same_open("eps = 0")
    assert select_both(math.inf, 5000, "eps = 0")["count"] > 50


def test_the_large_scenario_covers_what_it_claims():
    """The open-set part of tests/large_case.py on the array references alone (tests/test_table.py has the table part):
    what keeps the push and select tests of tests/test_gpu_table_large.py from being vacuous (they repeat it)."""
    gh = O.lattice_hash(2, O.ACC, LC.goal_row())
    sc, snaps = LC.reference(gh)
    LC.assert_open_conditions(sc, snaps, gh)


def test_every_function_of_the_header_is_declared_in_abi(engine):
    syms = _declared("mplx_open.h")
    assert "mplx_open_push_device" in syms and "mplx_open_select_device" in syms and len(syms) == 6
    assert sorted(engine._abi.OPEN_SYMBOLS) == syms
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s
    assert C.sizeof(engine._abi.OpenView) == 2 * 8 and C.sizeof(engine._abi.OpenResult) == 48
    assert (engine.search.IS_OPEN, engine.search.IS_GOAL, engine.search.SEEN) == (OM.IS_OPEN, OM.IS_GOAL, OM.SEEN)
    assert (engine.search.SELECTED, engine.search.FOUND, engine.search.EMPTY) == (OM.SELECTED, OM.FOUND, OM.EMPTY)
    assert (engine.search.MAX_ROUNDS, engine.search.MAX_EXPAND) == (OM.MAX_ROUNDS, OM.MAX_EXPAND)


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_open.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
