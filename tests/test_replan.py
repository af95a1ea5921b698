"""CPU: the semantics of include/mplx_replan.h as tests/replan_model.py restates them.  On the corridor of the
reference's test_planner_2d a replan -- after the robot has advanced along its path, after a wall has been put across
the path or taken away again, after the goal has moved -- ends at exactly the cost of a fresh search from the root on
the new map, in a fraction of its rounds; a hand-built table pins the corners of the rule (a bad edge in mid chain, a
stale child, a predecessor with a larger id, a seed that is not the root, roots that are none, a cycle).  Plus the
plumbing of the new header (declared in _abi.py, parses as C).  Successors and edges come from the CPU oracle; no GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import open_model as OM
import replan_model as RM
from oracle import oracle as O
from table_model import TableModel, oracle_provider
from test_plan_known_answer import corridor
from test_table import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, DELTA, CAP = 1.0, 10.0, 65536  # the first search: 351.5 in 35 rounds, 6 073 expansions, 10 102 nodes, 35 edges

# name -> what happens between the first search and the replan.  first: the map of the first search ("open": the
# corridor, "walled": with the wall across the path's middle edge); wall: the wall the map has at the replan (None, "mid":
# across the edge b -> b + 1 with b = len(path) // 2, "late": b = len(path) - 6); advance: the root is that node of the
# path (0: the seed); cap: max_frontier of the replan (the forced round's chunks AND the selections after it); goal: the
# goal moves by that many metres (cells of 0.05 m).
SCENARIOS = {
    "advance": dict(first="open", wall=None, advance=5),
    "advance_chunks": dict(first="open", wall=None, advance=5, cap=500),
    "wall_mid": dict(first="open", wall="mid", advance=0),
    "wall_mid_advance": dict(first="open", wall="mid", advance=5),
    "wall_late": dict(first="open", wall="late", advance=0),
    "unwall": dict(first="walled", wall=None, advance=0),
    "unwall_advance": dict(first="walled", wall=None, advance=5),
    "goal_moved": dict(first="open", wall=None, advance=5, goal=(-0.3, 0.2)),
}
# name -> nodes before, kept, bad edges, cost, rounds and expansions of the replan, rounds and expansions of the fresh
# search from the root: what the committed model gives.  The first seven are the issue's table but for one figure: with
# chunks of 500 rows the replan expands 4 264, not 5 816 -- max_frontier also cuts the one selection after the forced
# round to 500 rows (as on the device), the issue's prototype cut the forced round only.
PINNED = {
    "advance": (10102, 3764, 0, 351.5, 2, 5816, 30, 4823),
    "advance_chunks": (10102, 3764, 0, 351.5, 9, 4264, 30, 4823),
    "wall_mid": (10102, 9166, 14, 352.0, 12, 10074, 35, 6232),
    "wall_mid_advance": (10102, 2852, 14, 352.0, 12, 6995, 30, 4924),
    "wall_late": (10102, 9977, 13, 352.0, 3, 10065, 35, 6263),
    "unwall": (10434, 10434, 0, 351.5, 17, 10610, 35, 6073),
    "unwall_advance": (10434, 3809, 0, 351.5, 17, 6988, 30, 4823),
    "goal_moved": (10102, 3764, 0, 351.75, 5, 6230, 30, 4762),
}


class Corridor:
    """The corridor, its controls and goal, and the two walls (found once, on the path of the first search)."""

    def __init__(self, engine):
        c = corridor()
        self.c, self.dim, self.origin, self.res = c, c["dim"], c["origin"], c["res"]
        self.U = engine.workloads.grid_controls([-0.5, 0.0, 0.5], 2)  # test_planner_2d.cpp:49-53
        self.start = engine.Waypoint(2, engine.ACC, pos=c["start"]).to_row()
        self.goal = engine.Waypoint(2, engine.ACC, pos=c["goal"]).to_row()
        self.grid = np.array(c["cells"], dtype=np.int8)
        table, out = self.first("open")
        assert out["status"] == OM.FOUND and out["result"]["goal_g"] == 351.5
        ids = RM.path_ids(table, out["result"]["goal_id"])
        assert (out["rounds"], out["expanded"], table.n_nodes, len(ids) - 1) == (35, 6073, 10102, 35)
        pos = lambda i: table.state[ids[i]][:2]
        self.walls = {"mid": RM.wall_cells(self.dim, self.origin, self.res, pos(len(ids) // 2), pos(len(ids) // 2 + 1)),
                      "late": RM.wall_cells(self.dim, self.origin, self.res, pos(len(ids) - 6), pos(len(ids) - 5))}
        assert len(self.walls["mid"]) == len(self.walls["late"]) == 7
        assert int((self.grid[self.walls["mid"]] == 100).sum()) == 1  # (one of its cells is occupied already)

    def cells(self, wall):
        g = self.grid.copy()
        if wall is not None:
            g[self.walls[wall]] = 100
        return g

    def map_of(self, first):
        return self.cells("mid" if first == "walled" else None)

    def oenv(self, grid):
        return O.Env(2, O.ACC, self.U, grid, self.dim, self.origin, self.res, v_max=1.0, a_max=1.0, dt=1.0)

    def open_model(self, table, goal_row=None, grid=None):
        goal_row = self.goal if goal_row is None else goal_row
        ray = OM.ray_blocked(grid, self.dim, self.origin, self.res, goal_row[:2]) if grid is not None else None
        return OM.OpenModel(table, 2, goal_row, O.lattice_hash(2, O.ACC, goal_row), w=10.0, v_max=1.0, tol_pos=0.5, blocked=ray)

    def first(self, first):
        table = TableModel(10)
        out = RM.fresh(table, self.open_model(table), oracle_provider(O, self.oenv(self.map_of(first))), self.start,
                       [O.lattice_hash(2, O.ACC, self.start)], 0.0, EPS, DELTA, CAP)
        return table, out

    def goal_of(self, sc):
        goal = self.goal.copy()
        goal[:2] += sc.get("goal", (0.0, 0.0))
        return goal


_world = []


def world(engine):
    if not _world:
        _world.append(Corridor(engine))
    return _world[0]


def run_scenario(engine, name):
    """(nodes before, root id, its g, its state, the replan's output, the fresh search's, the table after the replan)."""
    w, sc = world(engine), SCENARIOS[name]
    table, out = w.first(sc["first"])
    ids = RM.path_ids(table, out["result"]["goal_id"])
    r = ids[sc["advance"]]
    g_root, s_root, n0 = table.g[r], table.state[r].copy(), table.n_nodes
    oenv, goal = w.oenv(w.cells(sc["wall"])), w.goal_of(sc)
    rp = RM.replan(table, w.open_model(table, goal), oracle_provider(O, oenv), RM.OracleEdges(O, oenv, table), len(w.U), EPS, DELTA,
                   sc.get("cap", CAP), root=r if sc["advance"] else -1)
    t2 = TableModel(10)
    fr = RM.fresh(t2, w.open_model(t2, goal), oracle_provider(O, oenv), s_root, [O.lattice_hash(2, O.ACC, s_root)], g_root, EPS, DELTA,
                  CAP)
    return n0, r, g_root, s_root, rp, fr, table


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_replan_ends_at_the_cost_of_a_fresh_search(engine, name):
    """FOUND, at the bits of the cost of a fresh search on the new map from the root's state, seeded with the root's g.
    Kept nodes, bad edges, rounds and expansions are pinned (PINNED says where they differ from the issue's table)."""
    sc = SCENARIOS[name]
    n0, r, g_root, s_root, rp, fr, table = run_scenario(engine, name)
    info = rp["info"]
    print(name, n0, info, rp["result"]["goal_g"], rp["rounds"], rp["expanded"], "fresh", fr["result"]["goal_g"], fr["rounds"],
          fr["expanded"])
    assert rp["status"] == OM.FOUND and fr["status"] == OM.FOUND
    assert np.float64(rp["result"]["goal_g"]).view(np.uint64) == np.float64(fr["result"]["goal_g"]).view(np.uint64)
    assert info["n_roots"] == 1 and info["n_kept"] >= 2  # a non-root node is kept
    if sc["wall"] is not None:
        assert info["n_bad_edges"] >= 1
    if name == "unwall":
        # Nothing CAN be dropped here, whatever the issue's guard asks: the root is the seed, every node has a finite g
        # and hangs below the seed, and taking cells away invalidates no edge.  What keeps the scenario from being
        # vacuous instead: the replan lowers the g of kept nodes (the path through the gap) and creates new ones.
        assert info["n_kept"] == n0 and info["n_bad_edges"] == 0
        assert table.n_nodes > n0 and rp["result"]["goal_g"] < 352.0
    else:
        assert info["n_kept"] < n0  # a node is dropped
    if name in PINNED:
        assert (n0, info["n_kept"], info["n_bad_edges"], rp["result"]["goal_g"], rp["rounds"], rp["expanded"], fr["rounds"],
                fr["expanded"]) == PINNED[name]
    assert rp["rounds"] < 0.6 * fr["rounds"]  # what the feature is for: the rounds (2 .. 17 against 30 .. 35), not the expansions
    # the chain of the goal node ends at the root, whose g it still carries
    chain = RM.path_ids(table, rp["result"]["goal_id"])
    assert chain[0] == (r if sc["advance"] else 0) and table.g[chain[0]] == g_root and table.pred[chain[0]] == -1


def test_the_moved_goal_scenario_moves_the_goal_region(engine):
    """The goal of "goal_moved" lies six cells from the old one in x and four in y: another lattice state ends the path."""
    w = world(engine)
    _, _, _, _, rp, fr, table = run_scenario(engine, "goal_moved")
    _, _, _, _, rp0, _, table0 = run_scenario(engine, "advance")
    a, b = table.state[rp["result"]["goal_id"]], table0.state[rp0["result"]["goal_id"]]
    assert rp["result"]["goal_g"] == fr["result"]["goal_g"] and (not np.array_equal(a[:2], b[:2]) or rp["result"]["goal_g"] != 351.5)
    assert np.abs(a[:2] - w.goal_of(SCENARIOS["goal_moved"])[:2]).max() <= 0.5


# ---- a hand-built table of 13 nodes and a fake edge function: every edge (p, a) leads to the node it created, at cost 1,
# except the blocked one and the two of the cycle (cost 0: no cycle of positive costs passes the edge test)
def hand_table():
    t = TableModel(10)
    #        id:  0    1    2    3    4    5    6    7    8     9    10   11   12
    t.g = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 2.5, 0.0, 1.0, 7.0, 7.0, 3.0, math.inf]
    t.pred = [-1, 0, 1, 2, 3, 4, 1, -1, 7, 10, 9, 12, -1]
    t.pred_action = [-1, 0, 0, 0, 0, 0, 1, -1, 0, 0, 0, 0, -1]
    t.hash = [100 + i for i in range(13)]
    t.state = [np.full(10, float(i)) for i in range(13)]
    t.ids = {h: i for i, h in enumerate(t.hash)}
    # 0 -> 1 -> 2 -> 3 -> 4 -> 5: the edge into 3 is bad (blocked), so 3, 4, 5 go
    # 6: a stale child of 1 (g 2.5 > g[1] + 1 = 2): kept.  1's pred is 0 < 1, 11's pred is 12 > 11
    # 7 -> 8: a second seed and its child (kept only when the roots are the seeds)
    # 9 <-> 10: a cycle of predecessors
    # 11 -> 12: a node whose predecessor has a LARGER id, and that predecessor was never reached (g = inf): both go, and
    # the edge counts as bad (inf + 1 > 3)
    return t


def hand_edge(p, a):
    child = {(0, 0): 1, (1, 0): 2, (2, 0): 3, (3, 0): 4, (4, 0): 5, (1, 1): 6, (7, 0): 8, (10, 0): 9, (9, 0): 10, (12, 0): 11}[(p, a)]
    if (p, a) == (2, 0):
        return 2, 100 + child, math.inf  # MPLX_SLOT_BLOCKED
    return RM.SLOT_FINITE, 100 + child, 0.0 if p in (9, 10) else 1.0


def test_hand_built_table():
    t = hand_table()
    fr, res, status = RM.rebase(t, hand_edge, 2, root=-1)
    assert status == 0 and res == {"n_kept": 6, "n_bad_edges": 2, "n_roots": 2}
    assert fr["id"].tolist() == [0, 1, 2, 6, 7, 8] and fr["g"].tolist() == [0.0, 1.0, 2.0, 2.5, 0.0, 1.0]
    assert [t.g[i] for i in (3, 4, 5, 9, 10, 11, 12)] == [math.inf] * 7
    assert [t.pred[i] for i in range(13)] == [-1, 0, 1, -1, -1, -1, 1, -1, 7, -1, -1, -1, -1]
    assert t.pred_action[6] == 1 and t.pred_action[3] == -1
    # the root is node 1: the seed 0 above it goes, and so does the other seed with its child
    t = hand_table()
    fr, res, _ = RM.rebase(t, hand_edge, 2, root=1)
    assert res == {"n_kept": 3, "n_bad_edges": 2, "n_roots": 1} and fr["id"].tolist() == [1, 2, 6]
    assert t.pred[1] == -1 and t.pred_action[1] == -1 and t.g[1] == 1.0 and t.g[0] == math.inf and t.g[7] == math.inf
    # a node whose predecessor has a larger id hangs below a root like any other
    t = hand_table()
    t.g[12] = 2.0
    fr, res, _ = RM.rebase(t, hand_edge, 2, root=12)
    assert fr["id"].tolist() == [11, 12] and res["n_roots"] == 1 and t.pred[11] == 12 and t.pred[12] == -1
    # without the edge test the blocked edge stays
    t = hand_table()
    fr, res, _ = RM.rebase(t, None, 0, root=-1, check_edges=False)
    assert fr["id"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8] and res["n_bad_edges"] == 0
    # roots that are none: out of range, a node with an infinite g, a node on the cycle (kept with what hangs below)
    for root, want in ((13, []), (10 ** 6, []), (12, []), (9, [9, 10])):
        t = hand_table()
        fr, res, _ = RM.rebase(t, hand_edge, 2, root=root)
        assert fr["id"].tolist() == want and res["n_roots"] == (1 if want else 0), root
        if not want:
            assert all(g == math.inf for g in t.g) and all(p == -1 for p in t.pred)
    # an action outside the control table and a successor that is another lattice state are bad edges
    t = hand_table()
    t.pred_action[8] = 2
    t.hash[6] = 999
    fr, res, _ = RM.rebase(t, hand_edge, 2, root=-1)
    assert fr["id"].tolist() == [0, 1, 2, 7] and res["n_bad_edges"] == 4
    # g[p] + cost > g[id]: the child claims less than its edge gives
    t = hand_table()
    t.g[2] = 1.5
    fr, res, _ = RM.rebase(t, hand_edge, 2, root=-1)
    assert fr["id"].tolist() == [0, 1, 6, 7, 8] and res["n_bad_edges"] == 3
    # a frontier too small
    t = hand_table()
    fr, res, status = RM.rebase(t, hand_edge, 2, root=-1, capacity=5)
    assert status == RM.FRONTIER_FULL and res["n_kept"] == 6 and fr["count"] == 5


def test_closed_push_sets_keys_and_goal_bits_only():
    t = hand_table()
    opn = OM.OpenModel(t, 2, np.full(10, 2.0), 102, 10.0, 1.0, tol_pos=0.5)
    fr, _, _ = RM.rebase(t, hand_edge, 2, root=-1)
    opn.push(RM.rows_of(fr, 0, 1), 1, 1.0)  # node 0 is open from before
    RM.push_closed(opn, RM.rows_of(fr, 1, 5), 4, 1.0)  # n_max cuts the last row
    assert opn.flags == {0: OM.SEEN | OM.IS_OPEN, 1: OM.SEEN, 2: OM.SEEN | OM.IS_GOAL, 6: OM.SEEN, 7: OM.SEEN}
    assert opn.f[2] == 2.0 and opn.f[1] == 1.0 + 10.0 * 1.0 and 8 not in opn.f
    res, _ = opn.select(0.0, 8)
    assert res["status"] == OM.FOUND and res["goal_id"] == 2  # a closed goal node takes part in the stopping rule


@pytest.mark.parametrize("world_key", [(2, 0x03, 56.0, 32), (3, 0x07, 46.0, 64)])
def test_the_edits_of_the_gpu_tests_are_meaningful(engine, world_key):
    """tests/test_gpu_replan.py::test_rebase_against_the_model chooses its cells and its root from the table the device
    made; the same choice on the model's table of the same search (the two are equal: tests/test_gpu_open.py) finds bad
    edges and keeps nodes below a root three edges down, in both small worlds."""
    from helpers import oracle_env
    from test_gpu_open import small_world_goal
    from test_gpu_replan import choose_edit, depths, oracle_env_with
    dim, control, g_max, edge = world_key
    wl, start, h0, goal = small_world_goal(engine, O, dim, control, g_max, edge)
    oe = oracle_env(wl)
    t = TableModel(4 * dim + 2)
    opn = OM.OpenModel(t, dim, goal, O.lattice_hash(dim, control, goal), oe.w, oe.v_max, tol_pos=wl.res,
                       blocked=OM.ray_blocked(wl.grid, wl.map_dim, wl.origin, wl.res, goal[:dim]))
    OM.search(t, opn, oracle_provider(O, oe), start, h0, 1.0, oe.w * oe.dt, 8192, sight=1, max_rounds=6)
    a = t.arrays()
    cells, r, grid = choose_edit(O, wl, a)
    assert len(cells) >= 3 and depths(t)[r] == 3
    for root in (r, -1):
        tt = RM.table_from_arrays(a)
        fr, info, _ = RM.rebase(tt, RM.OracleEdges(O, oracle_env_with(O, wl, grid), tt), len(wl.U), root=root)
        assert info["n_bad_edges"] >= 1 and 2 <= info["n_kept"] < t.n_nodes and info["n_roots"] == 1
        assert np.array_equal(fr["id"], np.sort(fr["id"]))


def test_every_function_of_the_header_is_declared_in_abi(engine):
    syms = _declared("mplx_replan.h")
    assert syms == ["mplx_open_push_closed_device", "mplx_table_rebase_device", "mplx_table_rebase_multi_device"]
    assert sorted(engine._abi.REPLAN_SYMBOLS) == syms
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s
    assert C.sizeof(engine._abi.RebaseResult) == 24
    assert hasattr(engine.table.NodeTable, "rebase") and hasattr(engine.search.SearchResult, "replan")
    assert hasattr(engine.search.MultiSearchResult, "replan")


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_replan.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
