"""GPU: include/mplx_prior.h against tests/prior_model.py, bit for bit: the prior table a launch builds (steps, positions,
remaining costs, the replaced goal), every push with it (open, closed, with the ray trace), the coarse-to-fine pipeline on
the corridor for one query and for eight, replanning with and without the priors, and that an open set without priors
gives the bytes it gave before."""
import ctypes as C
import math

import numpy as np
import pytest

import multi_model as MM
import open_model as OM
import prior_model as PM
import replan_model as RM
from table_model import TableModel, oracle_provider
from test_gpu_multi import assert_multi_table_equal
from test_gpu_open import assert_open_equal, assert_result_equal, corridor_env
from test_gpu_table import assert_table_equal, bits
from test_open import corridor_search
from test_plan_known_answer import corridor
from test_prior import _planner, first_plan, host_table, stage1  # noqa: F401 (first_plan is a fixture)

pytestmark = pytest.mark.gpu

VEL, JRK = 0x01, 0x07
W, VMAX = 10.0, 1.0


def grid_u(m):
    return m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)


def jrk_env(m, dt=1.0, cells=None, control=JRK, U=None):
    c = corridor()
    env = m.EnvMap(2)
    env.setMap(c["origin"], c["dim"], c["cells"] if cells is None else cells, c["res"])
    env.set_control(control)
    env.set_u(grid_u(m) if U is None else U)
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(dt)
    return env


def wp(m, control, pos):
    return m.Waypoint(2, control, pos=pos).to_row()


_coarse = {}


def coarse(m, shift=0.0):
    """The model's VEL stage on the corridor (tests/test_prior.py::stage1), for the start shifted by (0, shift) and the goal
    by (0, -shift): (start row, actions, U of the VEL stage, the search's output, nodes)."""
    if shift not in _coarse:
        c = corridor()
        if shift == 0.0:
            table, out, start, acts, U1 = stage1(m)
        else:
            from oracle import oracle as O
            U1 = 2.0 * grid_u(m)
            oenv = O.Env(2, O.VEL, U1, c["cells"], c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
            start, goal = wp(m, VEL, c["start"] + np.array([0.0, shift])), wp(m, VEL, c["goal"] - np.array([0.0, shift]))
            table = TableModel(10)
            opn = OM.OpenModel(table, 2, goal, O.lattice_hash(2, O.VEL, goal), w=W, v_max=VMAX, tol_pos=0.5)
            out = OM.search(table, opn, oracle_provider(O, oenv), start, O.lattice_hash(2, O.VEL, start), 1.0, 0.0, 65536)
            ids = RM.path_ids(table, out["result"]["goal_id"])
            acts = np.array([table.pred_action[i] for i in ids[1:]], dtype=np.int32)
        _coarse[shift] = (start, acts, U1, out, table.n_nodes)
    return _coarse[shift]


def model_prior(m, start, acts, dt=1.0, cells=None, pot=None, pot_w=0.0, grad_w=0.0, goal_row=None, goal_hash=None):
    c = corridor()
    return PM.prior_table(2, VEL, 2.0 * grid_u(m), 1.0, start, acts, c["cells"] if cells is None else cells, c["dim"], c["origin"],
                          c["res"], VMAX, W, dt, pot=pot, pot_w=pot_w, grad_w=grad_w, goal_row=goal_row, goal_hash=goal_hash)


def assert_prior_equal(got, q, want, what=""):
    assert got["n_steps"][q] == want["n_steps"], what
    assert np.array_equal(bits(got["pos"][q]), bits(want["pos"])), what + ": pos"
    assert np.array_equal(bits(got["togo"][q]), bits(want["togo"])), what + ": togo"
    assert np.array_equal(bits(got["goal_row"][q]), bits(want["goal_row"])), what + ": goal row"
    assert int(got["goal_hash"][q]) == int(want["goal_hash"]), what + ": goal hash"


# ---- 1. the table --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gradient_weight", [0.0, 0.25])
def test_build_six_priors_on_a_potential_map(engine, first_plan, gradient_weight):
    m, c = engine, corridor()
    first, start, path, U1 = first_plan  # the host planner's VEL plan: the device, the model and the host getter see one prior
    assert len(path) == 34
    env = jrk_env(m)
    pot = env.updatePotentialMap(c["start"], [1.0, 1.0])
    env.set_potential_weight(0.5)
    env.set_gradient_weight(gradient_weight)
    H = 40
    actions = np.full((H, 6), -1, np.int32)
    actions[:34, 0] = path                      # 0: the 34-segment VEL path
    actions[1:5, 1] = 7                         # 1: empty (the first action ends it)
    actions[:20, 2] = 7                         # 2: straight through a wall
    actions[:10, 3] = 1                         # 3: leaves the map
    actions[:34, 4] = path
    actions[12, 4] = 99                         # 4: a bad action in the middle
    actions[0, 5] = path[0]                     # 5: one segment
    goal = wp(m, JRK, c["goal"])
    goals = np.stack([goal] * 6)
    tab = env.alloc_table(64, n_queries=6)
    opn = env.alloc_open(tab)
    opn.set_goals(goals, tol_pos=0.5)
    assert opn.priors() is None
    info = opn.set_priors(start, actions, VEL, U1, 1.0)
    got = opn.priors()
    gh = PM.lattice_hash(2, JRK, goal)
    want = [model_prior(m, start, actions[:, q], cells=pot, pot=pot, pot_w=0.5, grad_w=gradient_weight, goal_row=goal, goal_hash=gh)
            for q in range(6)]
    print(info, [w_["n_steps"] for w_ in want], [w_["status"] for w_ in want])
    assert [w_["n_steps"] for w_ in want] == [34, 0, 20, 10, 12, 1]
    assert [w_["status"] for w_ in want] == [0, PM.EMPTY, 0, 0, PM.BAD_ACTION, 0]
    assert np.all(np.isinf(want[2]["togo"])) and np.all(np.isinf(want[3]["togo"])) and np.all(np.isfinite(want[0]["togo"]))
    assert info["status"].tolist() == [w_["status"] for w_ in want] and info["n_steps"].tolist() == [w_["n_steps"] for w_ in want]
    for q in range(6):
        assert_prior_equal(got, q, want[q], "query %d" % q)
    # the host planner's table of the same prior on the same potential map
    keep = []
    second = _planner(m, c, m.JRK, grid_u(m), pot, 1.0, keep)
    second.setW(10)
    second.setPriorTrajectory(first, potential=pot, potential_weight=0.5, gradient_weight=gradient_weight)
    host = host_table(m, second)
    second.close()
    assert host["n_steps"] == 34 and host["control"] == VEL
    for k in ("pos", "togo", "goal_row"):
        assert np.array_equal(bits(got[k][0]), bits(host[k])), k
    # clear_priors: no table, and set_goals drops one as well
    opn.clear_priors()
    assert opn.priors() is None
    opn.set_priors(start, actions, VEL, U1, 1.0)
    assert opn.priors() is not None
    opn.set_goals(goals, tol_pos=0.5)
    assert opn.priors() is None
    opn.free()
    tab.free()
    env.close()


def test_build_with_the_truncated_quotient(engine):
    m, c = engine, corridor()
    start, path, U1, _, _ = coarse(m)
    env = jrk_env(m, dt=0.1)
    goal = wp(m, JRK, c["goal"])
    tab = env.alloc_table(64)
    opn = env.alloc_open(tab)
    opn.set_goals(goal.reshape(1, -1), tol_pos=0.5)
    info = opn.set_priors(start, path.reshape(-1, 1), VEL, U1, 1.0)
    want = model_prior(m, start, path, dt=0.1)
    off = [k for k, t in enumerate(want["steps_t"]) if int(t / 0.1) != k]
    assert 8 in off and want["n_steps"] >= 340 and info["n_steps"][0] == want["n_steps"] and info["status"][0] == 0
    assert_prior_equal(opn.priors(), 0, want)
    opn.free()
    tab.free()
    env.close()


# ---- 2. the push ---------------------------------------------------------------------------------------------------------

def test_push_with_priors(engine, oracle_lib):
    """Three queries, query 1 without a prior; rows at t = 0, below and at a step boundary, the last step, one step past
    the prior's end, a negative and a NaN time, the priors' goal states themselves and rows inside the goal tolerance."""
    m, O, c = engine, oracle_lib, corridor()
    start, path, U1, _, _ = coarse(m)
    env = jrk_env(m)
    goal = wp(m, JRK, c["goal"])
    goals = np.stack([goal, goal, wp(m, JRK, c["goal"] - np.array([0.0, 0.5]))])
    short = path[:20]
    actions = np.full((34, 3), -1, np.int32)
    actions[:34, 0], actions[:20, 2] = path, short
    hashes = [O.lattice_hash(2, JRK, g) for g in goals]
    pri = [model_prior(m, start, path), None, model_prior(m, start, short)]
    assert pri[0]["n_steps"] == 34 and pri[2]["n_steps"] == 20
    times = [0.0, 0.5, 1.0, 19.0, 20.0, 33.0, 34.0, 35.0, -1.0, math.nan]
    cols, query = [], []
    for q in range(3):
        for j, t in enumerate(times):
            k = 0 if not t > 0 else min(int(t), 33)
            s = np.zeros(10)
            s[:2] = pri[0]["pos"][k] + [0.3 + 0.01 * j, -0.2]
            s[9] = t
            cols.append(s)
            query.append(q)
        ends = [pri[q]["goal_row"] if pri[q] else goals[q]]
        for j, d in enumerate([(0.0, 0.0), (0.25, 0.0), (0.0, -0.4), (0.6, 0.0)]):  # the goal state, inside, inside, outside
            s = np.array(ends[0], dtype=np.float64)
            s[2:8] = 0.0
            s[:2] += d
            s[9] = 33.0 + j
            cols.append(s)
            query.append(q)
    states = np.stack(cols, axis=1)
    query = np.array(query, dtype=np.int32)
    g = 0.25 * np.arange(states.shape[1])
    tab = env.alloc_table(256, n_queries=3)
    opn = env.alloc_open(tab)
    opn.set_goals(goals, tol_pos=0.5)
    info = opn.set_priors(start, actions, VEL, U1, 1.0)
    assert info["n_steps"].tolist() == [34, 0, 20]
    fr = m.TableFrontier(env, states.shape[1])
    count = tab.seed(states, g, frontier=fr, query=query)
    table = MM.MultiTableModel(10, 3)
    want_fr, _ = table.seed(states, [O.lattice_hash(2, JRK, states[:, i]) for i in range(states.shape[1])], g, query=query)
    assert count == want_fr["count"] == states.shape[1]
    assert_multi_table_equal(tab, table)
    eff = [pri[q]["goal_row"] if pri[q] else goals[q] for q in range(3)]
    blocked = [OM.ray_blocked(c["cells"], c["dim"], c["origin"], c["res"], eff[q][:2]) for q in range(3)]
    model = PM.PriorMultiOpenModel(table, 2, goals, hashes, W, VMAX, 1.0, pri, tol_pos=0.5, blocked=blocked)
    plain = MM.MultiOpenModel(table, 2, goals, hashes, W, VMAX, tol_pos=0.5)
    opn.push(fr, n_max=count, eps=1.0)
    model.push(want_fr, count, 1.0)
    plain.push(want_fr, count, 1.0)
    assert_open_equal(opn, model, "open push")
    f, fl = model.arrays()
    f0, _ = plain.arrays()
    assert (f != f0).sum() >= 12 and np.array_equal(f[query == 1], f0[query == 1])  # the prior moves keys, and only its queries'
    assert (fl & OM.IS_GOAL).sum() >= 6
    opn.clear()
    model.f, model.flags = {}, {}
    opn.push(fr, n_max=count, eps=2.0, closed=True)
    RM.push_closed(model, want_fr, count, 2.0)
    assert_open_equal(opn, model, "closed push")
    opn.clear()
    model.f, model.flags = {}, {}
    opn.push(fr, n_max=count, eps=1.0, sight=True)
    model.push(want_fr, count, 1.0, sight=1)
    assert_open_equal(opn, model, "push with sight")
    # without the priors: the keys of the plain open set again
    opn.clear_priors()
    opn.clear()
    opn.push(fr, n_max=count, eps=1.0)
    assert_open_equal(opn, plain, "after clear_priors")
    fr.free()
    opn.free()
    tab.free()
    env.close()


# ---- 3. the search -------------------------------------------------------------------------------------------------------

_fine = {}


def fine_model(m, O, delta, prior):
    """The JRK-state stage on the model (tests/test_prior.py::stage2, kept with its table and open set)."""
    key = (delta, prior is not None)
    if key not in _fine:
        from test_prior import stage2
        _fine[key] = stage2(m, delta, prior)
    return _fine[key]


def vel_stage(m):
    c = corridor()
    env = jrk_env(m, control=VEL, U=2.0 * grid_u(m))
    r = env.search(wp(m, VEL, c["start"]), wp(m, VEL, c["goal"]), eps=1.0, delta=0.0, capacity=1 << 12, sight=False)
    return env, r


@pytest.mark.parametrize("delta", [0.0, 10.0])
def test_two_stage_search_of_one_query(engine, oracle_lib, delta):
    m, O, c = engine, oracle_lib, corridor()
    start1, path, U1, out1, nodes1 = coarse(m)
    env1, r1 = vel_stage(m)
    assert r1.found and r1.cost == 382.0 and (r1.rounds, r1.expanded, r1.table.stats()[0]) == (out1["rounds"], out1["expanded"], nodes1)
    prior = r1.as_prior()
    assert np.array_equal(prior.actions, path) and np.array_equal(bits(prior.start), bits(start1))
    assert prior.control == VEL and prior.dt == 1.0 and np.array_equal(prior.U, U1)
    env = jrk_env(m)
    start, goal = wp(m, JRK, c["start"]), wp(m, JRK, c["goal"])
    r2 = env.search(start, goal, eps=1.0, delta=delta, capacity=1 << 16, sight=False, prior=prior)
    table, opn, want = fine_model(m, O, delta, model_prior(m, start1, path))
    print(delta, r2, r2.last_select, want["rounds"], want["expanded"], table.n_nodes)
    assert r2.status == m.search.FOUND == want["status"] and (r2.rounds, r2.expanded) == (want["rounds"], want["expanded"])
    assert_result_equal(r2.last_select, want["result"])
    assert r2.cost == 353.25 and r2.last_select["goal_f"] == 358.25
    assert_table_equal(r2.table, table)
    assert_open_equal(r2.open, opn)
    s0, act = r2.path()
    ro = env.rollout(s0, act.reshape(-1, 1))
    assert ro["status"][0] == m.SLOT_FINITE and ro["steps"][0] == len(act) == 35 and bits(ro["cost"])[0] == bits([r2.cost])[0]
    r1.free()
    r2.free()
    env1.close()
    env.close()


def test_two_stage_search_of_eight_queries(engine, oracle_lib):
    """Eight queries (the corridor's own and the one shifted by 0.5 m, alternating), two of them without a prior."""
    m, O, c = engine, oracle_lib, corridor()
    Q, shifts, none = 8, [0.0, 0.5] * 4, (2, 5)
    s0, g0 = np.asarray(c["start"], dtype=np.float64), np.asarray(c["goal"], dtype=np.float64)
    env1 = jrk_env(m, control=VEL, U=2.0 * grid_u(m))
    r1 = env1.search_many(np.stack([wp(m, VEL, s0 + [0.0, sh]) for sh in shifts], axis=1),
                          np.stack([wp(m, VEL, g0 - [0.0, sh]) for sh in shifts]), eps=1.0, delta=0.0, capacity=1 << 13, sight=False)
    assert all(r1.found)
    priors = r1.as_priors()
    pri = []
    for q in range(Q):
        st, acts, U1, _, _ = coarse(m, shifts[q])
        assert np.array_equal(priors[q].actions, acts) and np.array_equal(bits(priors[q].start), bits(st)), q
        pri.append(None if q in none else model_prior(m, st, acts))
    for q in none:
        priors[q] = None
    env = jrk_env(m)
    starts = np.stack([wp(m, JRK, s0 + [0.0, sh]) for sh in shifts], axis=1)
    goals = np.stack([wp(m, JRK, g0 - [0.0, sh]) for sh in shifts])
    r2 = env.search_many(starts, goals, eps=1.0, delta=0.0, capacity=1 << 17, sight=False, priors=priors)
    oenv = O.Env(2, O.JRK, grid_u(m), c["cells"], c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    table = MM.MultiTableModel(10, Q)
    model = PM.PriorMultiOpenModel(table, 2, goals, [O.lattice_hash(2, O.JRK, g) for g in goals], W, VMAX, 1.0, pri, tol_pos=0.5)
    want = MM.search_many(table, model, oracle_provider(O, oenv), starts, [O.lattice_hash(2, O.JRK, starts[:, q]) for q in range(Q)],
                          1.0, 0.0, 1 << 17)
    print(r2, r2.rounds, r2.expanded, r2.cost)
    assert r2.status == want["status"] == [OM.FOUND] * Q and want["truncated"] == 0
    assert (r2.rounds, r2.expanded, r2.total_rounds) == (want["rounds"], want["expanded"], want["total_rounds"])
    for q in range(Q):
        assert_result_equal(r2.last_select[q], want["results"][q], "query %d" % q)
        assert r2.cost[q] == (363.0 if q in none else 353.25) or shifts[q] != 0.0
        st, act = r2.path(q)
        ro = env.rollout(st, act.reshape(-1, 1))
        assert ro["status"][0] == m.SLOT_FINITE and ro["steps"][0] == len(act) and bits(ro["cost"])[0] == bits([r2.cost[q]])[0], q
    assert r2.expanded[0] < r2.expanded[2] and r2.cost[0] <= r2.cost[2]  # the same query with and without its prior
    assert_multi_table_equal(r2.table, table)
    assert_open_equal(r2.open, model)
    r1.free()
    r2.free()
    env1.close()
    env.close()


# ---- 4. replanning -------------------------------------------------------------------------------------------------------

def test_replan_keeps_the_priors_and_a_new_goal_drops_them(engine, oracle_lib):
    m, O, c = engine, oracle_lib, corridor()
    start1, path, U1, _, _ = coarse(m)
    prior = m.search.Prior(start1, path, VEL, U1, 1.0)
    pm = model_prior(m, start1, path)
    env = jrk_env(m)
    start, goal = wp(m, JRK, c["start"]), wp(m, JRK, c["goal"])
    cap = 1 << 15
    r2 = env.search(start, goal, eps=1.0, delta=0.0, capacity=cap, sight=False, prior=prior)
    assert r2.found and r2.cost == 353.25
    d0 = r2.table.download()
    ids, _ = r2.table.path(r2.goal_id)
    cells = RM.wall_cells(c["dim"], c["origin"], c["res"], d0["state"][:2, ids[8]], d0["state"][:2, ids[9]])
    grid = np.array(c["cells"], dtype=np.int8)
    grid[cells] = 100
    env.editMap(cells, 100)
    oenv = O.Env(2, O.JRK, grid_u(m), grid, c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    # with the priors the open set keeps
    t = RM.table_from_arrays(d0)
    mo = PM.PriorOpenModel(t, 2, goal, O.lattice_hash(2, O.JRK, goal), W, VMAX, 1.0, prior=pm, tol_pos=0.5)
    want = RM.replan(t, mo, oracle_provider(O, oenv), RM.OracleEdges(O, oenv, t), 9, 1.0, 0.0, cap, root=int(ids[3]))
    r3 = r2.replan(advance=3)
    print(r3, r3.rebase_info, want["info"], want["rounds"], want["expanded"])
    assert r3.open.priors() is not None and r3.open.priors()["n_steps"][0] == 34
    assert r3.status == want["status"] == OM.FOUND and (r3.rounds, r3.expanded) == (want["rounds"], want["expanded"])
    assert (r3.rebase_info["n_kept"], r3.rebase_info["n_bad_edges"]) == (want["info"]["n_kept"], want["info"]["n_bad_edges"])
    assert r3.rebase_info["n_bad_edges"] >= 1
    assert_result_equal(r3.last_select, want["result"])
    assert_table_equal(r3.table, t)
    assert_open_equal(r3.open, mo)
    # a new goal: the priors are gone, the goal is the open set's own
    goal2 = wp(m, JRK, c["goal"] - np.array([0.0, 0.5]))
    d1 = r3.table.download()
    t2 = RM.table_from_arrays(d1)
    mo2 = PM.PriorOpenModel(t2, 2, goal2, O.lattice_hash(2, O.JRK, goal2), W, VMAX, 1.0, prior=None, tol_pos=0.5)
    want2 = RM.replan(t2, mo2, oracle_provider(O, oenv), RM.OracleEdges(O, oenv, t2), 9, 1.0, 0.0, cap)
    r4 = r3.replan(goal_row=goal2)
    print(r4, r4.rebase_info, want2["rounds"], want2["expanded"])
    assert r4.open.priors() is None
    assert r4.status == want2["status"] and (r4.rounds, r4.expanded) == (want2["rounds"], want2["expanded"])
    assert_result_equal(r4.last_select, want2["result"])
    assert_table_equal(r4.table, t2)
    assert_open_equal(r4.open, mo2)
    r4.free()
    env.close()


# ---- 5. no change --------------------------------------------------------------------------------------------------------

def test_without_priors_the_bytes_are_those_of_the_search_before(engine):
    """EnvMap.search on the corridor as tests/test_gpu_open.py runs it, and the same loop on an open set that was given
    goals of its own, priors, and clear_priors(): one table, one open set, the model's."""
    m = engine
    S = m.search
    env, start, goal = corridor_env(m)
    table, model, want = corridor_search(m, 1.0, 10.0, 4096, sight=1)
    res = env.search(start, goal, capacity=1 << 15, max_frontier=4096)
    assert res.status == S.FOUND and res.cost == 351.5 and (res.rounds, res.expanded) == (want["rounds"], want["expanded"])
    assert_table_equal(res.table, table)
    assert_open_equal(res.open, model)
    a, fa = res.table.download(), res.open.download()
    # the loop of EnvMap.search on an open set that had priors once
    st1, path, U1, _, _ = coarse(m)
    prm = S._params(env, 1.0, 10.0, math.inf, None, None, 1 << 15, 4096, None, True, dict(tol_pos=0.5))
    tab = env.alloc_table(1 << 15)
    opn = env.alloc_open(tab)
    opn.set_goals(goal.reshape(1, -1), tol_pos=0.5)
    opn.set_priors(st1, path.reshape(-1, 1), VEL, U1, 1.0)
    assert opn.priors()["n_steps"][0] == 34
    opn.clear_priors()
    sel, imp = m.TableFrontier(env, 4096), m.TableFrontier(env, 1 << 15)
    lists = env.alloc_lists(4096, want_state=True)
    count = tab.seed(start, None, frontier=imp)
    opn.push(imp, n_max=count, eps=1.0, sight=True)
    rounds, expanded = [0], [0]
    status, last, total = S._search_loop(env, "search", False, tab, opn, sel, imp, lists, prm, 0, rounds, expanded)
    assert status[0] == S.FOUND and (total, expanded[0]) == (res.rounds, res.expanded)
    assert_result_equal(last[0], res.last_select)
    b, fb = tab.download(), opn.download()
    assert a["n_nodes"] == b["n_nodes"]
    for k in ("hash", "g", "pred", "pred_action", "state"):
        assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), k
    assert np.array_equal(fa["flags"], fb["flags"])
    seen = (fa["flags"] & OM.SEEN) > 0
    assert np.array_equal(bits(fa["f"][seen]), bits(fb["f"][seen]))
    for x in (sel, imp, lists):
        x.free()
    opn.free()
    tab.free()
    res.free()
    env.close()


# ---- 6. errors -----------------------------------------------------------------------------------------------------------

def test_argument_errors_and_state(engine):
    m, c = engine, corridor()
    L_, ARG, STATE, OK = m._abi.lib(), m._abi.ERR_ARG, m._abi.ERR_STATE, m._abi.OK
    start, path, U1, _, _ = coarse(m)
    env = jrk_env(m)
    goal = wp(m, JRK, c["goal"])
    d_start, d_act, d_U = m.DeviceArray(env, 80), m.DeviceArray(env, 4 * 34), m.DeviceArray(env, U1.nbytes)
    d_start.upload(start)
    d_act.upload(path)
    d_U.upload(U1)

    def call(o, n_traj=1, horizon=34, U=d_U.ptr, nU=9, udim=2, dt=1.0, control=VEL, src=True, tset=True):
        s = m._abi.TrajSet()
        s.starts, s.n_starts, s.start_stride, s.actions = d_start.ptr, 1, 1, d_act.ptr
        s.n_traj, s.horizon, s.action_stride = n_traj, horizon, max(n_traj, 1)
        p = m._abi.PriorSource()
        p.control, p.nU, p.udim, p.U, p.dt = control, nU, udim, U, dt
        return L_.mplx_open_set_priors_device(o._open if o is not None else None, C.byref(p) if src else None,
                                              C.byref(s) if tset else None, None)
    tab = env.alloc_table(64)
    opn = env.alloc_open(tab)
    assert call(opn) == STATE  # no goals of its own yet (the context's goal does not count)
    env.set_goal(goal)
    assert call(opn) == STATE
    opn.set_goals(goal.reshape(1, -1), tol_pos=0.5)
    assert call(None) == ARG and call(opn, src=False) == ARG and call(opn, tset=False) == ARG
    assert call(opn, n_traj=2) == ARG and call(opn, n_traj=0) == ARG
    assert call(opn, horizon=0) == ARG
    assert call(opn, U=None) == ARG and call(opn, nU=0) == ARG and call(opn, udim=1) == ARG and call(opn, control=0x05) == ARG
    for dt in (0.0, -1.0, math.nan, math.inf):
        assert call(opn, dt=dt) == ARG, dt
    assert opn.priors() is None  # nothing of the above built anything
    env.set_v_max(-1.0)
    env._flush()
    assert call(opn) == STATE
    env.set_v_max(1.0)
    env._flush()
    assert call(opn) == OK and opn.priors()["n_steps"][0] == 34
    assert L_.mplx_open_prior_view_of(opn._open, None) == ARG and L_.mplx_open_prior_view_of(None, None) == ARG
    opn.free()
    tab.free()
    env.close()
    # no map
    env = m.EnvMap(2)
    env.set_control(JRK)
    env.set_u(grid_u(m))
    env.set_v_max(1.0)
    env.set_dt(1.0)
    env._flush()
    tab = env.alloc_table(64)
    opn = env.alloc_open(tab)
    opn.set_goals(goal.reshape(1, -1), tol_pos=0.5)
    d2 = [m.DeviceArray(env, 80), m.DeviceArray(env, 4 * 34), m.DeviceArray(env, U1.nbytes)]
    d_start, d_act, d_U = d2
    assert call(opn, U=d_U.ptr) == STATE and opn.priors() is None
    with pytest.raises(m._abi.MplxError) as err:
        opn.set_priors(start, path.reshape(-1, 1), VEL, U1, 1.0)
    assert err.value.code == STATE
    with pytest.raises(ValueError):
        opn.set_prior_list([None, None])
    opn.free()
    tab.free()
    env.close()
