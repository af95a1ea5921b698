"""CPU: include/mplx_prior.h as tests/prior_model.py restates it.  The model's prior table equals the host planner's
(mplx_planner_prior_table: the restatement the reference's prior-trajectory scenario pins) bit for bit, without and with
a potential map and on the truncated-quotient case; on the corridor the guided second stage of a coarse-to-fine plan
expands fewer nodes than the unguided one for a better path.  Successors come from the CPU oracle; no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import open_model as OM
import prior_model as PM
from oracle import oracle as O
from table_model import TableModel, oracle_provider
from test_plan_known_answer import corridor, provider_from_oracle
from test_table import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_prior.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_every_function_of_the_header_is_exported_and_bound(engine):
    syms = _declared("mplx_prior.h")
    assert syms == sorted(["mplx_open_set_priors_device", "mplx_open_clear_priors", "mplx_open_prior_view_of", "mplx_planner_prior_table"])
    assert sorted(engine._abi.PRIOR_SYMBOLS) == syms
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s
    assert C.sizeof(engine._abi.PriorSource) == 32 and C.sizeof(engine._abi.PriorInfo) == 16 and C.sizeof(engine._abi.PriorView) == 48
    assert lib.mplx_abi_version() == 9
    for name in ("set_priors", "clear_priors", "priors"):
        assert hasattr(engine.search.OpenSet, name)
    assert hasattr(engine.search.SearchResult, "as_prior") and hasattr(engine.search.MultiSearchResult, "as_priors")
    # the entry points check their arguments before they touch a device
    assert lib.mplx_open_set_priors_device(None, None, None, None) == engine._abi.ERR_ARG
    assert lib.mplx_open_clear_priors(None) == engine._abi.ERR_ARG
    assert lib.mplx_planner_prior_table(None, None, None, 0, None, None, None) == engine._abi.ERR_ARG


# ---- the host planner's table (the scenario of tests/test_plan_known_answer.py) against the model ----------------------

def _planner(m, c, control, U, cells, dt, keep, dim=2):
    oenv = O.Env(dim, control, U, cells, c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=dt)
    prov, ce = provider_from_oracle(oenv)
    keep.append((oenv, ce))
    pl = m.MapPlanner(dim, provider=prov)
    mu = m.MapUtil(dim)
    mu.setMap(c["origin"], c["dim"], cells, c["res"])
    pl.setMapUtil(mu)
    pl.setVmax(1.0)
    pl.setAmax(1.0)
    pl.setDt(dt)
    pl.setU(U)
    return pl


def host_table(m, planner, dim=2):
    L = m._abi.lib()
    n, ctl = C.c_int32(), C.c_int32()
    assert L.mplx_planner_prior_table(planner._p, None, None, 0, C.byref(n), None, None) == 0
    pos, togo, goal = np.zeros((n.value, dim)), np.zeros(n.value), np.zeros(4 * dim + 2)
    assert L.mplx_planner_prior_table(planner._p, pos.ctypes.data, togo.ctypes.data, n.value, C.byref(n), goal.ctypes.data, C.byref(ctl)) == 0
    return {"n_steps": n.value, "pos": pos, "togo": togo, "goal_row": goal, "control": ctl.value}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_table(model, host, what=""):
    assert model["n_steps"] == host["n_steps"], what
    assert np.array_equal(bits(model["pos"]), bits(host["pos"])), what
    assert np.array_equal(bits(model["togo"]), bits(host["togo"])), what
    assert np.array_equal(bits(model["goal_row"]), bits(host["goal_row"])), what


@pytest.fixture(scope="module")
def first_plan(engine):
    """The VEL plan of test_planner_2d_with_prior_traj.cpp:47-58 on the host planner (unit controls, dt = 1)."""
    m, c, keep = engine, corridor(), []
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    first = _planner(m, c, m.VEL, 2.0 * U, c["cells"], 1.0, keep)
    assert first.plan(m.Waypoint(2, m.VEL, pos=c["start"]), m.Waypoint(2, m.VEL, pos=c["goal"]))
    tr = first.getTraj()
    yield first, np.array(tr.nodes[0]), np.array(tr.actions, dtype=np.int32), 2.0 * U
    first.close()


@pytest.mark.parametrize("potential, gradient_weight", [(False, 0.0), (True, 0.0), (True, 0.25)])
def test_the_model_table_is_the_host_planners_bit_for_bit(engine, first_plan, potential, gradient_weight):
    m, c, keep = engine, corridor(), []
    first, start, actions, U1 = first_plan
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    pot = O.update_potential_map(c["cells"], c["dim"], c["origin"], c["res"], c["start"], [1.0, 1.0]) if potential else None
    cells = pot if potential else c["cells"]
    second = _planner(m, c, m.JRK, U, cells, 1.0, keep)
    second.setW(10)
    if potential:
        second.setPriorTrajectory(first, potential=pot, potential_weight=0.5, gradient_weight=gradient_weight)
    else:
        second.setPriorTrajectory(first)
    host = host_table(m, second)
    second.close()
    model = PM.prior_table(2, m.VEL, U1, 1.0, start, actions, cells, c["dim"], c["origin"], c["res"], 1.0, 10.0, 1.0,
                           pot=pot, pot_w=0.5, grad_w=gradient_weight)
    assert host["n_steps"] == len(actions) > 30 and host["control"] == m.VEL
    assert_same_table(model, host, (potential, gradient_weight))
    assert np.all(np.isfinite(model["togo"])) and model["togo"][0] == model["total_cost"]
    if potential:  # the potential term is in the table: the remaining cost is no longer w * (T - t)
        plain = PM.prior_table(2, m.VEL, U1, 1.0, start, actions, c["cells"], c["dim"], c["origin"], c["res"], 1.0, 10.0, 1.0)
        assert not np.array_equal(model["togo"], plain["togo"])
    assert model["goal_hash"] == O.lattice_hash(2, O.VEL, model["goal_row"])


def test_the_truncated_quotient_indexes_the_costs(engine, first_plan):
    """dt = 0.1 in the searching planner: t_k accumulates rounding error and (int)(t_k / dt) is not k for some steps --
    k = 8 (t_8 = 0.7999999999999999 -> 7) is one of them; model and host agree on every entry."""
    m, c, keep = engine, corridor(), []
    first, start, actions, U1 = first_plan
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    second = _planner(m, c, m.JRK, U, c["cells"], 0.1, keep)
    second.setW(10)
    second.setPriorTrajectory(first)
    host = host_table(m, second)
    second.close()
    model = PM.prior_table(2, m.VEL, U1, 1.0, start, actions, c["cells"], c["dim"], c["origin"], c["res"], 1.0, 10.0, 0.1)
    assert model["T"] >= 0.9
    off = [k for k, t in enumerate(model["steps_t"]) if int(t / 0.1) != k]
    assert 8 in off and model["steps_t"][8] == 0.7999999999999999
    assert model["togo"][8] == model["total_cost"] - 10.0 * model["steps_t"][7]  # costs[7], not costs[8]
    assert_same_table(model, host)


def test_edge_cases_of_the_table():
    c = corridor()
    U = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])
    start = np.zeros(10)
    start[:2] = c["start"]
    args = (c["cells"], c["dim"], c["origin"], c["res"], 1.0, 10.0, 1.0)
    goal = np.arange(10.0)
    e = PM.prior_table(2, 1, U, 1.0, start, [-1, 0], *args, goal_row=goal, goal_hash=5)
    assert e["status"] == PM.EMPTY and e["n_steps"] == 0 and np.array_equal(e["goal_row"], goal) and e["goal_hash"] == 5
    b = PM.prior_table(2, 1, U, 1.0, start, [0, 0, 9, 0], *args)
    assert b["status"] == PM.BAD_ACTION and b["n_steps"] == 2 and b["T"] == 2.0
    out = PM.prior_table(2, 1, U, 1.0, start, [2] * 40, *args)  # leaves the map: traverse = +inf
    assert out["n_steps"] == 40 and np.all(np.isinf(out["togo"]))
    one = PM.prior_table(2, 1, U, 1.0, start, [0], *args)
    assert one["n_steps"] == 1 and one["togo"][0] == 10.0 and one["goal_row"][0] == start[0] + 1.0 and one["goal_row"][9] == 0.0


# ---- the open set with priors on the corridor: coarse to fine ----------------------------------------------------------

def stage1(engine):
    """The VEL search with U = {-1, 0, 1}^2 under the open set's batch rule, and its path as a prior."""
    m, c = engine, corridor()
    U1 = 2.0 * m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    oenv = O.Env(2, O.VEL, U1, c["cells"], c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    start = m.Waypoint(2, m.VEL, pos=c["start"]).to_row()
    goal = m.Waypoint(2, m.VEL, pos=c["goal"]).to_row()
    table = TableModel(10)
    opn = OM.OpenModel(table, 2, goal, O.lattice_hash(2, O.VEL, goal), w=10.0, v_max=1.0, tol_pos=0.5)
    out = OM.search(table, opn, oracle_provider(O, oenv), start, O.lattice_hash(2, O.VEL, start), 1.0, 0.0, 65536)
    acts, i = [], out["result"]["goal_id"]
    while table.pred[i] >= 0:
        acts.append(int(table.pred_action[i]))
        i = table.pred[i]
    return table, out, start, np.array(acts[::-1], dtype=np.int32), U1


def stage2(engine, delta, prior, start_pos=None, cells=None):
    m, c = engine, corridor()
    grid = c["cells"] if cells is None else cells
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    oenv = O.Env(2, O.JRK, U, grid, c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    start = m.Waypoint(2, m.JRK, pos=c["start"] if start_pos is None else start_pos).to_row()
    goal = m.Waypoint(2, m.JRK, pos=c["goal"]).to_row()
    table = TableModel(10)
    opn = PM.PriorOpenModel(table, 2, goal, O.lattice_hash(2, O.JRK, goal), 10.0, 1.0, 1.0, prior=prior, tol_pos=0.5)
    out = OM.search(table, opn, oracle_provider(O, oenv), start, O.lattice_hash(2, O.JRK, start), 1.0, delta, 65536)
    return table, opn, out


@pytest.fixture(scope="module")
def coarse(engine):
    c = corridor()
    table, out, start, acts, U1 = stage1(engine)
    prior = PM.prior_table(2, O.VEL, U1, 1.0, start, acts, c["cells"], c["dim"], c["origin"], c["res"], 1.0, 10.0, 1.0)
    return table, out, start, acts, U1, prior


def test_stage_one_is_the_vel_plan(coarse):
    table, out, start, acts, U1, prior = coarse
    res = out["result"]
    print("stage 1", out["status"], res["goal_g"], out["rounds"], out["expanded"], table.n_nodes, len(acts), prior["goal_row"][:2])
    assert out["status"] == OM.FOUND and res["goal_g"] == 382.0
    assert (out["rounds"], out["expanded"], table.n_nodes) == (42, 245, 268)
    assert len(acts) == 34 and tuple(prior["goal_row"][:2]) == (36.5, 2.5) and prior["n_steps"] == 34


# (delta, guided) -> goal_g, goal_f, rounds, expanded, nodes: what the committed model gives
STAGE2 = {
    (0.0, True): (353.25, 358.25, 79, 1275, 3819),
    (0.0, False): (363.0, 363.0, 96, 3006, 8296),
    (10.0, True): (353.25, 358.25, 36, 12959, 31372),
    (10.0, False): (363.0, 363.0, 36, 28961, 68799),
}
_runs = {}


def run_stage2(engine, coarse, case):
    if case not in _runs:
        delta, guided = case
        table, opn, out = stage2(engine, delta, coarse[5] if guided else None)
        i, edges = out["result"]["goal_id"], 0
        while i >= 0 and table.pred[i] >= 0:
            i, edges = table.pred[i], edges + 1
        _runs[case] = (out, table.n_nodes, i, edges)
    return _runs[case]


@pytest.mark.parametrize("case", sorted(STAGE2))
def test_stage_two_guided_and_unguided(engine, coarse, case):
    out, nodes, root, edges = run_stage2(engine, coarse, case)
    res = out["result"]
    got = (res["goal_g"], res["goal_f"], out["rounds"], out["expanded"], nodes)
    print(case, out["status"], got)
    assert out["status"] == OM.FOUND and out["truncated"] == 0
    assert got == STAGE2[case]
    # the chain of best predecessors has as many edges as goal_g implies: every edge costs w * dt = 10 plus an effort < 10
    assert root == 0 and edges == int(res["goal_g"] // 10.0)


def test_the_prior_buys_expansions_and_a_better_path(engine, coarse):
    g, u = run_stage2(engine, coarse, (0.0, True)), run_stage2(engine, coarse, (0.0, False))
    assert g[0]["status"] == u[0]["status"] == OM.FOUND
    assert g[0]["expanded"] < u[0]["expanded"] and g[1] < u[1]
    assert g[0]["rounds"] * g[0]["expanded"] < u[0]["rounds"] * u[0]["expanded"]
    assert g[0]["result"]["goal_g"] <= u[0]["result"]["goal_g"]
