"""CPU: tests/anytime_model.py (the sequential rule of include/mplx_anytime.h) against tables worked out by hand, and the
arithmetic of SearchResult.bound.  No engine, no GPU."""
import math

import numpy as np
import pytest

import anytime_model as AM
import multi_model as MM
import open_model as OM

O, G, S = OM.IS_OPEN, OM.IS_GOAL, OM.SEEN
W, VMAX = 2.0, 1.0


class Stub:
    def __init__(self, hashes, g, state, query, Q):
        self.hash, self.g, self.state, self.query = hashes, g, state, query
        self.n_nodes, self.n_queries, self.n_fields = len(hashes), Q, state.shape[0]


def hand():
    """Two queries, goals (4, 0) and (0, 3), w = 2, v_max = 1 (h = 2 * Linf).  Five nodes:
         id  query  pos     g     flags          h   L = g + h
         0   0      (0, 0)  1     SEEN|OPEN      8   9
         1   0      (4, 0)  5     SEEN|OPEN|GOAL 0   5      the goal's own lattice state (its hash): h = 0
         2   0      (2, 0)  3     SEEN           4   7      closed
         3   1      (0, 1)  2.5   SEEN|OPEN      4   6.5
         4   1      (9, 9)  0     0              -   -      never pushed"""
    state = np.zeros((10, 5))
    state[:2] = [[0, 4, 2, 0, 9], [0, 0, 0, 1, 9]]
    goals = np.zeros((2, 10))
    goals[0, :2], goals[1, :2] = (4, 0), (0, 3)
    t = Stub([10, 111, 12, 13, 14], [1.0, 5.0, 3.0, 2.5, 0.0], state, [0, 0, 0, 1, 1], 2)
    m = MM.MultiOpenModel(t, 2, goals, [111, 222], W, VMAX, tol_pos=0.5)
    m.f = {0: 1.0 + 3 * 8, 1: 5.0, 2: 3.0 + 3 * 4, 3: 2.5 + 3 * 4}  # as pushed with eps = 3
    m.flags = {0: S | O, 1: S | O | G, 2: S, 3: S | O}
    return t, m


def test_rekey_with_a_tie_at_the_cut():
    t, m = hand()
    out = AM.rekey(m, 2.0, True, [9.0, math.inf], 2)
    assert m.f == {0: 17.0, 1: 5.0, 2: 11.0, 3: 10.5}
    # node 0 sits exactly on the cut of its query: pruned; the closed node 2 (L = 7 < 9) is not counted; +inf prunes nothing
    assert m.flags == {0: S, 1: S | O | G, 2: S, 3: S | O}
    assert out == [{"lower": 5.0, "n_open": 2, "n_pruned": 1, "n_rekeyed": 3}, {"lower": 6.5, "n_open": 1, "n_pruned": 0, "n_rekeyed": 1}]
    assert 4 not in m.f and 4 not in m.flags


def test_a_cut_just_above_the_tie_prunes_nothing_and_eps_zero_gives_g():
    t, m = hand()
    out = AM.rekey(m, 0.0, True, [math.nextafter(9.0, math.inf), 0.0], 2)
    assert m.f == {0: 1.0, 1: 5.0, 2: 3.0, 3: 2.5}
    assert m.flags == {0: S | O, 1: S | O | G, 2: S, 3: S}  # a cut of 0 closes every open node of query 1
    assert [b["n_pruned"] for b in out] == [0, 1] and [b["lower"] for b in out] == [5.0, 6.5]  # lower: before any pruning


def test_write_zero_changes_nothing_and_still_bounds():
    t, m = hand()
    f0, fl0 = dict(m.f), dict(m.flags)
    out = AM.rekey(m, 1.0, False, [0.0, 0.0], 2)
    assert m.f == f0 and m.flags == fl0
    assert out == [{"lower": 5.0, "n_open": 2, "n_pruned": 0, "n_rekeyed": 0}, {"lower": 6.5, "n_open": 1, "n_pruned": 0, "n_rekeyed": 0}]


def test_an_empty_open_set_and_an_empty_table():
    t, m = hand()
    m.flags[3] = S  # query 1 has nothing open
    out = AM.rekey(m, 1.0, True, None, 2)
    assert out[1] == {"lower": math.inf, "n_open": 0, "n_pruned": 0, "n_rekeyed": 1} and m.f[3] == 6.5
    t.n_nodes = 0
    assert AM.rekey(m, 1.0, True, None, 2) == [{"lower": math.inf, "n_open": 0, "n_pruned": 0, "n_rekeyed": 0}] * 2


def test_a_key_that_is_not_a_number_stays_and_bounds_nothing():
    t, m = hand()
    h_of = lambda i, s: math.nan if i == 0 else m.heur_and_tol(i, s)[0]  # (what ROBUST gives for a non-finite row)
    out = AM.rekey(m, 2.0, True, [0.0, math.inf], 2, h_of=h_of)
    assert m.f[0] == 25.0 and m.flags[0] == S | O  # key kept, not pruned (NaN >= cut is false) ...
    assert out[0] == {"lower": 5.0, "n_open": 2, "n_pruned": 1, "n_rekeyed": 2}  # ... but counted as open; node 1 is pruned


def test_identity_at_the_eps_of_the_pushes():
    t, m = hand()
    f0, fl0 = dict(m.f), dict(m.flags)
    AM.rekey(m, 3.0, True, None, 2)
    assert m.f == f0 and m.flags == fl0


def test_argument_errors():
    t, m = hand()
    for eps in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            AM.rekey(m, eps, True, None, 2)
    for cut in ([math.nan, 1.0], [1.0, -0.5], [1.0]):
        with pytest.raises(ValueError):
            AM.rekey(m, 1.0, True, cut, 2)


def test_bound_arithmetic():
    s = AM.slack_of(10.0, 2.0, 0.5)
    assert s == 2.5 and AM.slack_of(10.0, 0.0, 0.5) == 5.0
    b = AM.bound(12.0, 11.0, math.inf, s, True)
    assert b["lower"] == 8.5 and b["ratio"] == 12.0 / 8.5
    assert AM.bound(12.0, 11.0, 9.0, s, True)["lower"] == 6.5           # g_max cuts the tree: no bound above it
    assert AM.bound(12.0, 1.0, math.inf, s, True) == {"cost": 12.0, "lower": 0.0, "slack": 2.5, "ratio": math.inf, "certified": True}
    u = AM.bound(12.0, 11.0, math.inf, s, False)
    assert u["lower"] == 8.5 and math.isnan(u["ratio"])                  # not certified: the number, but no ratio
    assert AM.bound(12.0, math.inf, math.inf, 0.0, True)["ratio"] == 0.0  # nothing open, nothing pruned: the tree is exhausted
    p = AM.bound(12.0, math.inf, math.inf, s, True, pruned_at=12.0 + s)    # everything open was pruned at cost + slack
    assert p["lower"] == 12.0 and p["ratio"] == 1.0


def test_schedule_on_the_corridor_models(engine):
    """The scenario of tests/test_gpu_anytime.py::test_schedule_on_the_corridor on the sequential models (successors from
    the CPU oracle): eps = 4, then improve to 2 and 1 with pruning at cost + slack.  The models themselves meet what the
    GPU test asserts: costs never rise, lower - slack <= the fresh eps = 1 cost at every stage, and the final cost is
    within slack of it."""
    from test_open import corridor_search, corridor_setup

    delta, cap, slack = 10.0, 1 << 16, AM.slack_of(10.0, 1.0, 0.5)
    _, _, fresh = corridor_search(engine, 1.0, delta, cap, sight=1)
    c, table, opn, prov, start, h0 = corridor_setup(engine, blocked=True)
    out = OM.search(table, opn, prov, start, h0, 4.0, delta, cap, sight=1)
    assert out["status"] == OM.FOUND and fresh["status"] == OM.FOUND and fresh["result"]["goal_g"] == 351.5
    pruned_at, seen = math.inf, []
    for eps in (4.0, 2.0, 1.0):
        if eps != 4.0:
            cut = out["result"]["goal_g"] + slack
            pruned_at = min(pruned_at, cut)
            out = AM.improve(table, opn, prov, eps, delta, cap, out["rounds"], out["expanded"], cut=[cut], sight=1)
            assert out["status"] == OM.FOUND
        lower = AM.rekey(opn, eps, False, None, 1)[0]["lower"]
        seen.append((eps, out["result"]["goal_g"], AM.bound(out["result"]["goal_g"], lower, math.inf, slack, True, pruned_at)))
    print(fresh["expanded"], [(e, c, b["lower"], b["ratio"]) for e, c, b in seen], out["expanded"])
    costs = [c for _, c, _ in seen]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    for eps, cost, b in seen:
        assert b["lower"] - slack <= fresh["result"]["goal_g"]
    assert abs(costs[-1] - fresh["result"]["goal_g"]) <= slack


def test_schedule_on_the_wall_map_models(engine):
    """tests/test_gpu_anytime.py::test_schedule_on_the_wall_map on the models: 48 x 32 cells, zero tolerances, w = 1,
    delta = 0, eps = 4, 2, 1.  Costs never rise, cost <= eps * lower at every stage, and the schedule ends at the bits of
    the fresh eps = 1 cost with ratio <= 1."""
    from oracle import oracle as O
    from table_model import TableModel, oracle_provider

    dims = [48, 32]
    U = engine.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    oenv = O.Env(2, O.ACC, U, AM.wall_cells(dims), dims, [0.0, 0.0], 0.25, dt=1.0, w=1.0, v_max=1.0, a_max=1.0)
    p0, p1 = AM.wall_query(dims)
    start, goal = engine.Waypoint(2, engine.ACC, pos=p0).to_row(), engine.Waypoint(2, engine.ACC, pos=p1).to_row()
    h0, cap = O.lattice_hash(2, O.ACC, start), 1 << 16

    def setup():
        table = TableModel(10)
        return table, OM.OpenModel(table, 2, goal, O.lattice_hash(2, O.ACC, goal), w=1.0, v_max=1.0, tol_pos=0.0)

    t1, o1 = setup()
    fresh = OM.search(t1, o1, oracle_provider(O, oenv), start, h0, 1.0, 0.0, cap)
    table, opn = setup()
    prov = oracle_provider(O, oenv)
    out = OM.search(table, opn, prov, start, h0, 4.0, 0.0, cap)
    assert fresh["status"] == OM.FOUND and out["status"] == OM.FOUND
    pruned_at, seen = math.inf, []
    for eps in (4.0, 2.0, 1.0):
        if eps != 4.0:
            cut = out["result"]["goal_g"]  # (slack 0)
            pruned_at = min(pruned_at, cut)
            out = AM.improve(table, opn, prov, eps, 0.0, cap, out["rounds"], out["expanded"], cut=[cut])
            assert out["status"] == OM.FOUND
        lower = AM.rekey(opn, eps, False, None, 1)[0]["lower"]
        seen.append((eps, AM.bound(out["result"]["goal_g"], lower, math.inf, 0.0, True, pruned_at), out["expanded"]))
    print("fresh", fresh["result"]["goal_g"], fresh["expanded"], [(e, b["cost"], b["lower"], b["ratio"], x) for e, b, x in seen])
    costs = [b["cost"] for _, b, _ in seen]
    assert all(b <= a for a, b in zip(costs, costs[1:])) and costs[0] > costs[-1]  # the schedule does improve something
    for eps, b, _ in seen:
        assert b["cost"] <= eps * b["lower"] * (1 + 1e-12)
    assert np.float64(costs[-1]).view(np.uint64) == np.float64(fresh["result"]["goal_g"]).view(np.uint64)
    assert seen[-1][1]["ratio"] <= 1 + 1e-12
