"""GPU: EnvMap.search / search_many / replan with heur="robust" (include/mplx_heur.h) on the exact-goal scenarios of
tests/heur_model.py: the device search equals the model's search loop round for round, finds the default search's cost
(both heuristics are admissible for a goal STATE with zero tolerances; costs are sums of binary fractions, so equality
is exact) and expands fewer nodes."""
import functools

import numpy as np
import pytest

import heur_model as HM
import open_model as OM
from test_gpu_table import assert_table_equal

pytestmark = pytest.mark.gpu

KW = dict(eps=1.0, delta=1.0, sight=False, tol_pos=0.0, tol_vel=0.0, capacity=1 << 15, max_frontier=1 << 13)


def scene_env(m, cells=None, D=2):
    env = m.EnvMap(D)
    if D == 2:
        env.setMap([0.0, 0.0], HM.SCENE_DIMS, HM.scene_cells() if cells is None else cells, HM.SCENE_RES)
        env.set_control(m.ACC)
    else:
        env.setMap([0.0] * 3, HM.SCENE3_DIMS, HM.scene3_cells(), HM.SCENE_RES)
        env.set_control(m.JRK)
        env.set_j_max(1.0)
    env.set_u(m.workloads.grid_controls([-1.0, 0.0, 1.0], D))
    env.set_w(HM.SCENE_W)
    env.set_v_max(HM.SCENE_VMAX)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    return env


@functools.lru_cache(maxsize=None)
def model(O, m, heur, start=HM.SCENE_START, goal=HM.SCENE_GOAL):
    """The model's search, once per (heuristic, query), shared by the tests and left unchanged."""
    return HM.scene_search(O, m, heur, start=start, goal=goal)


def assert_same_search(res, want, table=None):
    out = want["result"]
    assert (res.status, res.rounds, res.expanded) == (want["status"], want["rounds"], want["expanded"])
    assert res.goal_id == out["goal_id"] and res.cost == out["goal_g"]
    for k in ("status", "goal_id", "count", "n_open", "f_min", "goal_f", "goal_g"):
        assert res.last_select[k] == out[k], k
    if table is not None:
        assert_table_equal(res.table, table)  # g, predecessors and actions of every node: the path with them


def test_search_with_robust_equals_the_model_and_beats_the_default(engine, oracle_lib):
    m, O = engine, oracle_lib
    t_r, _, want_r = model(O, m, HM.ROBUST)
    t_d, _, want_d = model(O, m, None)
    # the scenario, on the models alone
    assert want_r["status"] == want_d["status"] == OM.FOUND
    assert want_r["result"]["goal_g"] == want_d["result"]["goal_g"] and want_r["expanded"] < want_d["expanded"]
    assert want_r["truncated"] == 0 and want_r["rounds"] >= 10
    env = scene_env(m)
    s, g = HM.scene_rows()
    plain = env.search(s[:, 0], g[0], **KW)
    robust = env.search(s[:, 0], g[0], heur="robust", **KW)
    print("default:", plain, "robust:", robust)
    assert_same_search(plain, want_d, t_d)
    assert_same_search(robust, want_r, t_r)
    assert robust.cost == plain.cost and robust.expanded < plain.expanded
    ids, act = robust.table.path(robust.goal_id)
    assert ids[0] == 0 and ids[-1] == robust.goal_id and len(act) >= 5
    # the goal node is the goal's own lattice state: its key is its g
    assert robust.last_select["goal_f"] == robust.cost
    plain.free()
    robust.free()
    env.close()


QUERIES = [(HM.SCENE_START, HM.SCENE_GOAL), ((6.25, 9.25), (15.25, 4.25)), ((3.25, 2.25), (13.25, 13.25))]


def test_search_many_with_robust(engine, oracle_lib):
    """Three queries in one table: each does what its own search does (the model's), and fewer expansions than the default."""
    m, O = engine, oracle_lib
    env = scene_env(m)
    s, g = HM.scene_rows([q[0] for q in QUERIES], [q[1] for q in QUERIES])
    kw = dict(KW, capacity=1 << 17)
    plain = env.search_many(s, g, **kw)
    robust = env.search_many(s, g, heur="robust", **kw)
    print("default:", plain, "robust:", robust)
    for q, (a, b) in enumerate(QUERIES):
        want_r, want_d = model(O, m, HM.ROBUST, a, b)[2], model(O, m, None, a, b)[2]
        for res, want in ((robust, want_r), (plain, want_d)):
            assert (res.status[q], res.rounds[q], res.expanded[q], res.cost[q]) == \
                (want["status"], want["rounds"], want["expanded"], want["result"]["goal_g"]), q
        assert robust.status[q] == OM.FOUND and robust.cost[q] == plain.cost[q] and robust.expanded[q] < plain.expanded[q]
    plain.free()
    robust.free()
    env.close()


def test_search_3d_jrk_with_robust(engine, oracle_lib):
    m, O = engine, oracle_lib
    t_r, _, want_r = HM.scene3_search(O, m, HM.ROBUST)
    t_d, _, want_d = HM.scene3_search(O, m, None)
    assert want_r["status"] == want_d["status"] == OM.FOUND and want_r["expanded"] < want_d["expanded"]
    env = scene_env(m, D=3)
    s, g = np.zeros(14), np.zeros(14)
    s[:3], g[:3] = HM.SCENE3_START, HM.SCENE3_GOAL
    kw = dict(KW, tol_acc=0.0, capacity=1 << 16)
    plain = env.search(s, g, **kw)
    robust = env.search(s, g, heur="robust", **kw)
    print("3D JRK default:", plain, "robust:", robust)
    assert_same_search(plain, want_d)
    assert_same_search(robust, want_r, t_r)
    assert robust.cost == plain.cost and robust.expanded < plain.expanded
    plain.free()
    robust.free()
    env.close()


def test_replan_keeps_the_mode(engine, oracle_lib):
    """After two steps along the path and a map edit that opens a shorter way, replan() pushes with ROBUST still: its
    keys are those of a fresh open set with the mode, and its cost is that of a fresh ROBUST search from the root."""
    m = engine
    env = scene_env(m)
    s, g = HM.scene_rows()
    r0 = env.search(s[:, 0], g[0], heur="robust", **KW)
    assert r0.found
    ids, act = r0.table.path(r0.goal_id)
    root_state = r0.table.state_of(ids[2])
    g_root = float(r0.table.download()["g"][ids[2]])
    new = HM.scene_cells(gap=True)
    changed = np.nonzero(new != HM.scene_cells())[0]
    env.editMap(changed, new[changed])
    r1 = r0.replan(advance=2)
    assert r0.table is None and r1.found
    root_state[-1] = 0.0  # (a fresh search starts its clock at the root)
    fresh = env.search(root_state, g[0], heur="robust", start_g=g_root, **KW)
    fresh_plain = env.search(root_state, g[0], start_g=g_root, **KW)
    print("replan:", r0.cost, "->", r1, "fresh:", fresh, "fresh default:", fresh_plain)
    assert fresh.found and r1.cost == fresh.cost == fresh_plain.cost
    # the mode is still in force: the keys of the kept nodes are ROBUST's, not the default's
    d, o = r1.table.download(), r1.open.download()
    n = d["n_nodes"]
    seen = (o["flags"][:n] & OM.SEEN) != 0
    h = HM.heur_eval(d["state"][:, :n], g[0], m.ACC, 0, HM.SCENE_W, HM.SCENE_VMAX, 2, HM.ROBUST)
    h0 = HM.heur_eval(d["state"][:, :n], g[0], m.ACC, 0, HM.SCENE_W, HM.SCENE_VMAX, 2, HM.DEFAULT)
    f = d["g"][:n] + 1.0 * h
    assert seen.sum() > 50 and np.array_equal(o["f"][:n][seen].view(np.uint64), (f[seen] + 0.0).view(np.uint64))
    assert np.sum(h[seen] > h0[seen]) > seen.sum() // 2
    for x in (r1, fresh, fresh_plain):
        x.free()
    env.close()
