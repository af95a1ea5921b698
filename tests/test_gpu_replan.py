"""GPU: include/mplx_replan.h on the device against tests/replan_model.py -- the rebase of a node table bit for bit
(table arrays, kept frontier, result), the closed push, and SearchResult.replan / MultiSearchResult.replan end to end
against a fresh search on the edited map.  The model is fed with the device's own table (download), so what is compared
is the rebase alone; its edges come from the CPU oracle on the edited map."""
import ctypes as C
import math

import numpy as np
import pytest

import control_matrix as CM
import multi_model as MM
import open_model as OM
import replan_model as RM
from helpers import engine_env
from table_model import TableModel, oracle_provider
from test_gpu_open import (OLD_WORLDS, assert_open_equal, assert_spare_untouched, corridor_env, patterned_frontier, rest_env,
                           small_world_goal)
from test_gpu_parity import _small_world
from test_gpu_table import assert_frontier_equal, bits
from test_multi import corridor_queries
from test_replan import CAP, DELTA, EPS, PINNED, SCENARIOS, world
from test_table import small_start

pytestmark = pytest.mark.gpu


# ---- helpers (no GPU needed: tests/test_replan.py::test_the_edits_of_the_gpu_tests_are_meaningful runs them on the model)
def cell_index(map_dim, origin, res, pos):
    """x + dim0 * (y + dim1 * z) of the cell that holds `pos`."""
    c = np.floor((np.asarray(pos, dtype=np.float64)[:len(map_dim)] - np.asarray(origin, dtype=np.float64)) / res).astype(int)
    idx, mul = 0, 1
    for i, d in enumerate(map_dim):
        idx, mul = idx + int(c[i]) * mul, mul * int(d)
    return idx


def depths(t):
    out = []
    for i in range(t.n_nodes):
        k, c = 0, i
        while t.pred[c] >= 0 and k <= t.n_nodes:
            c, k = t.pred[c], k + 1
        out.append(k)
    return out


def oracle_env_with(O, wl, grid):
    return O.Env(wl.dim, wl.control, wl.U, grid, wl.map_dim, wl.origin, wl.res, potential=wl.potential, region=wl.region,
                 **wl.params)


def choose_edit(O, wl, arrays, n_cells=5):
    """(cells to block, root): the cells under a handful of nodes two to four edges below the seed that have children
    (never the seed's own cell), and a root three edges down a chain such that the model, on the edited map, finds bad
    edges and still keeps a node below that root.  Chosen on the CPU, from the table the device made."""
    t = RM.table_from_arrays(arrays)
    d = depths(t)
    has_child = set(p for p in t.pred if p >= 0)
    seed_cell = cell_index(wl.map_dim, wl.origin, wl.res, t.state[0])
    cand = [i for i in range(t.n_nodes) if 2 <= d[i] <= 4 and i in has_child]
    cells = []
    for i in cand[::max(len(cand) // n_cells, 1)]:
        c = cell_index(wl.map_dim, wl.origin, wl.res, t.state[i])
        if c != seed_cell and c not in cells and len(cells) < n_cells:
            cells.append(c)
    grid = np.array(wl.grid, dtype=np.int8).ravel().copy()
    grid[cells] = 100
    oenv = oracle_env_with(O, wl, grid)
    for r in [i for i in range(t.n_nodes) if d[i] == 3 and i in has_child][:40]:
        tt = RM.table_from_arrays(arrays)
        _, info, _ = RM.rebase(tt, RM.OracleEdges(O, oenv, tt), len(wl.U), root=r)
        if info["n_bad_edges"] >= 1 and info["n_kept"] >= 2 and info["n_kept"] < t.n_nodes - 1:
            return cells, r, grid
    raise AssertionError("no root three edges down keeps a node on the edited map")


def restore(m, tab, d):
    """g, pred and pred_action of a download() back into the table (a rebase changes nothing else)."""
    v, n = tab.view(), d["n_nodes"]
    for ptr, a in ((v.g, d["g"]), (v.pred, d["pred"]), (v.pred_action, d["pred_action"])):
        a = np.ascontiguousarray(a[:n])
        m._abi.check(tab._env._ctx, m._abi.lib().mplx_memcpy_h2d(tab._env._ctx, int(ptr), a.ctypes.data, a.nbytes))


def assert_rebased_equal(tab, model, what=""):
    """The node arrays after a rebase, against the model's."""
    got, want = tab.download(), model.arrays()
    assert got["status"] == 0 and got["n_nodes"] == want["n_nodes"], what
    assert np.array_equal(got["hash"], want["hash"]), what + ": hash"
    assert np.array_equal(bits(got["g"]), bits(want["g"])), what + ": g"
    assert np.array_equal(got["pred"], want["pred"]), what + ": pred"
    assert np.array_equal(got["pred_action"], want["pred_action"]), what + ": pred_action"
    assert np.array_equal(bits(got["state"]), bits(want["state"])), what + ": state"
    return got


def rebase_both(m, env, tab, d0, edges_of, nU, what, root=-1, roots=None, check_edges=True, cap=None, spare=32, n_queries=1):
    """Restores the table to d0, rebases on the device and in the model and compares everything.  Returns (device
    frontier, model frontier, model table, result)."""
    restore(m, tab, d0)
    model = RM.table_from_arrays(d0, n_queries)
    want_fr, want, status = RM.rebase(model, edges_of(model) if check_edges else None, nU, root=root, roots=roots,
                                      check_edges=check_edges)
    assert status == 0
    fr = patterned_frontier(m, env, d0["n_nodes"] if cap is None else cap, spare)
    got = tab.rebase(root=root, roots=roots, check_edges=check_edges, frontier=fr)
    assert got == want, "%s: %r != %r" % (what, got, want)
    assert_frontier_equal(fr.download(), want_fr, what)
    assert int(fr.count.download(np.int64, (1,))[0]) == want["n_kept"], what
    assert_rebased_equal(tab, model, what)
    # rows past the count are not written
    n, k = fr.state_stride, want["n_kept"]
    from test_gpu_open import PAT_D, PAT_I
    assert np.all(fr.id.download(np.int32, (n,))[k:] == PAT_I) and np.all(fr.g.download(np.float64, (n,))[k:] == PAT_D), what
    assert np.all(fr.state.download(np.float64, (fr.n_fields, n))[:, k:] == PAT_D), what
    assert_spare_untouched(fr, what)
    return fr, want_fr, model, want


# ---- 1. rebase against the model on the two small worlds
@pytest.mark.parametrize("world_key", OLD_WORLDS + [pytest.param(CM.SNP_WORLD, id="2d-snp"), pytest.param(CM.SNP_WORLD_3D, id="3d-snp")])
def test_rebase_against_the_model(engine, oracle_lib, world_key):
    m, O = engine, oracle_lib
    dim, control, g_max, edge = world_key
    wl, start, h0, goal = small_world_goal(m, O, dim, control, g_max, edge)
    env = engine_env(m, wl)
    res = env.search(start, goal, max_rounds=6, capacity=1 << 14, max_frontier=8192, tol_pos=wl.res)
    tab, opn = res.table, res.open
    d0 = tab.download()
    assert d0["status"] == 0 and d0["n_nodes"] > 300
    cells, r, grid = choose_edit(O, wl, d0)
    env.editMap(cells, 100)
    oenv, nU = oracle_env_with(O, wl, grid), len(wl.U)
    edges_of = lambda model: RM.OracleEdges(O, oenv, model)
    for root in (r, -1):
        for check in (True, False):
            what = "root %d check %d" % (root, check)
            fr, want_fr, model, info = rebase_both(m, env, tab, d0, edges_of, nU, what, root=root, check_edges=check)
            if check:
                assert info["n_bad_edges"] >= 1 and info["n_kept"] >= 2, what  # bad edges, and a non-root node is kept
            else:
                assert info["n_bad_edges"] == 0, what
            fr.free()
    # a frontier of exactly n_kept rows, with patterned spare rows behind it
    fr, want_fr, model, info = rebase_both(m, env, tab, d0, edges_of, nU, "exact", root=r)
    fr.free()
    fr, want_fr, model, info = rebase_both(m, env, tab, d0, edges_of, nU, "exact", root=r, cap=info["n_kept"])
    # the closed push with the ray trace: a goal among the kept nodes, so that some carry IS_GOAL
    k = info["n_kept"] // 2
    near = np.zeros(4 * dim + 2)
    near[:dim] = want_fr["state"][:dim, k]
    env.set_goal(near, tol_pos=3 * wl.res)
    om = OM.OpenModel(model, dim, near, O.lattice_hash(dim, control, near), env._p.w, env._p.v_max, tol_pos=3 * wl.res,
                      blocked=OM.ray_blocked(grid, wl.map_dim, wl.origin, wl.res, near[:dim]))
    opn.clear()
    opn.push(fr, n_max=info["n_kept"], eps=1.5, sight=True, closed=True)
    RM.push_closed(om, want_fr, info["n_kept"], 1.5, 1)
    assert_open_equal(opn, om, "closed push")
    flags = np.array(list(om.flags.values()))
    assert len(om.flags) == info["n_kept"] and not (flags & OM.IS_OPEN).any() and (flags & OM.IS_GOAL).any()
    sel = m.TableFrontier(env, 64)
    got = opn.select(0.0, sel)
    assert got["status"] == OM.FOUND and got["count"] == 0  # closed goal nodes take part in the stopping rule
    # ... and the same rows pushed open: the plain push is what it was
    opn.push(fr, n_max=info["n_kept"], eps=1.5, sight=True)
    om.push(want_fr, info["n_kept"], 1.5, 1)
    assert_open_equal(opn, om, "open push")
    fr.free()
    sel.free()
    # one row too few
    restore(m, tab, d0)
    short = m.TableFrontier(env, info["n_kept"] - 1)
    got = tab.rebase(root=r, frontier=short)
    assert got["n_kept"] == info["n_kept"] and tab.stats()[1] & m.table.FRONTIER_FULL
    assert int(short.count.download(np.int64, (1,))[0]) == info["n_kept"] - 1
    with pytest.raises(m._abi.MplxError) as err:
        tab.rebase(root=r, frontier=short)
    assert err.value.code == m._abi.ERR_STATE
    short.free()
    res.free()
    env.close()


# ---- 2. a chain of more than 100 edges
def tunnel(m):
    """A 2D tunnel three free cells (0.75 m) wide and 115 m long, the corridor's controls; start and goal 110 m apart."""
    res, md = 0.25, [460, 5]
    grid = np.zeros((md[1], md[0]), np.int8)
    grid[0, :] = grid[4, :] = 100
    env = m.EnvMap(2)
    env.setMap([0.0, 0.0], md, grid.ravel(), res)
    env.set_control(m.ACC)
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    env.set_u(U)
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    start = m.Waypoint(2, m.ACC, pos=[0.625, 0.625]).to_row()
    goal = m.Waypoint(2, m.ACC, pos=[110.625, 0.625]).to_row()
    return env, start, goal, grid.ravel().copy(), md, res, U


def test_deep_chain(engine, oracle_lib):
    m, O = engine, oracle_lib
    env, start, goal, grid, md, res, U = tunnel(m)
    r = env.search(start, goal, eps=1.0, delta=10.0, capacity=1 << 16, sight=False)
    assert r.found
    tab = r.table
    ids, act = tab.path(r.goal_id)
    assert len(act) >= 100  # 7 doubling passes and more
    d0 = tab.download()
    n = d0["n_nodes"]
    mid = (d0["state"][:2, ids[2]] + d0["state"][:2, ids[3]]) / 2
    cell = cell_index(md, [0.0, 0.0], res, mid)
    env.editMap([cell], 100)
    g1 = grid.copy()
    g1[cell] = 100
    oenv = lambda g: O.Env(2, O.ACC, U, g, md, [0.0, 0.0], res, v_max=1.0, a_max=1.0, dt=1.0)
    fr, want_fr, model, info = rebase_both(m, env, tab, d0, lambda t: RM.OracleEdges(O, oenv(g1), t), len(U), "blocked")
    on_path = set(int(i) for i in ids[3:])
    assert info["n_bad_edges"] >= 1 and all(model.g[i] == math.inf for i in on_path)  # everything behind the cell goes
    assert 2 <= info["n_kept"] < n and any(model.pred[i] >= 0 for i in range(n))       # nodes beside the chain stay
    assert len([i for i in range(n) if model.g[i] == math.inf]) >= 100
    fr.free()
    # the cell is free again: nothing is bad, and only what the first rebase dropped stays dropped
    env.editMap([cell], 0)
    d1 = tab.download()
    fr, want_fr2, model2, info2 = rebase_both(m, env, tab, d1, lambda t: RM.OracleEdges(O, oenv(grid), t), len(U), "cleared")
    assert info2["n_bad_edges"] == 0 and info2["n_kept"] == info["n_kept"] and np.array_equal(want_fr2["id"], want_fr["id"])
    fr.free()
    r.free()
    env.close()


# ---- 3. several tiles: the corridor's 10 102 nodes
def corridor_edges(O, w, grid):
    oenv = w.oenv(grid)
    return lambda t: RM.OracleEdges(O, oenv, t)


def test_rebase_over_several_tiles(engine, oracle_lib):
    m, O = engine, oracle_lib
    w = world(m)
    env, start, goal = corridor_env(m)
    r = env.search(start, goal, eps=EPS, delta=DELTA, capacity=1 << 15, sight=False)
    d0 = r.table.download()
    assert r.cost == 351.5 and d0["n_nodes"] == 10102 and (r.rounds, r.expanded) == (35, 6073)  # three tiles of ids
    ids, _ = r.table.path(r.goal_id)
    env.editMap(w.walls["mid"], 100)
    fr, want_fr, model, info = rebase_both(m, env, r.table, d0, corridor_edges(O, w, w.cells("mid")), len(w.U), "advance 5",
                                           root=int(ids[5]))
    assert (d0["n_nodes"], info["n_kept"], info["n_bad_edges"]) == PINNED["wall_mid_advance"][:3]
    assert want_fr["id"][-1] > 2 * 4096
    fr.free()
    r.free()
    env.close()


# ---- 4. a table of three queries
def test_rebase_of_three_queries(engine, oracle_lib):
    m, O = engine, oracle_lib
    w = world(m)
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    r = env.search_many(starts, goals, eps=EPS, delta=DELTA, capacity=1 << 16, sight=False)
    assert all(r.found) and r.cost == [351.5, 351.75, 352.0]
    tab = r.table
    d0 = tab.download()
    q = d0["query"]
    assert any(len(set(q[i:i + 64])) > 1 for i in range(0, d0["n_nodes"] - 64, 64))  # a wave holds several queries
    ids0, _ = tab.path(r.goal_id[0])
    # the wall across q0's 4th edge crosses the path of no other query
    cells = RM.wall_cells(w.dim, w.origin, w.res, d0["state"][:2, ids0[3]], d0["state"][:2, ids0[4]])
    grid = w.grid.copy()
    grid[cells] = 100
    env.editMap(cells, 100)
    edges_of = corridor_edges(O, w, grid)
    t = RM.table_from_arrays(d0, 3)
    E = edges_of(t)
    blocked = []
    for k in range(3):
        p, _ = tab.path(r.goal_id[k])
        blocked.append(sum(E(int(a), t.pred_action[int(c)])[0] != RM.SLOT_FINITE for a, c in zip(p[:-1], p[1:])))
    assert blocked[0] >= 1 and blocked[1] == blocked[2] == 0
    other = int(ids0[7])  # a node of q0: no root for q2
    roots = [int(ids0[5]), -1, other]
    fr, want_fr, model, info = rebase_both(m, env, tab, d0, edges_of, len(w.U), "three queries", roots=roots, n_queries=3)
    kq = q[want_fr["id"]]
    assert info["n_roots"] == 2 and info["n_bad_edges"] >= 1
    assert (kq == 2).sum() == 0 and 2 <= (kq == 0).sum() < (q == 0).sum()
    # q1 keeps everything whose edges survive: all of it but what hangs below a bad edge
    assert 0.9 * (q == 1).sum() < (kq == 1).sum() <= (q == 1).sum()
    fr.free()
    # the plain call refuses a table of several queries
    with pytest.raises(m._abi.MplxError) as err:
        tab.rebase(root=-1, frontier=m.TableFrontier(env, 8))
    assert err.value.code == m._abi.ERR_STATE
    r.free()
    env.close()


# ---- 5. end to end
def rollout_cost(m, env, res):
    start_state, act = res.path()
    out = env.rollout(start_state, act.reshape(-1, 1))
    assert out["status"][0] == m.SLOT_FINITE and out["steps"][0] == len(act)
    return float(out["cost"][0])


@pytest.mark.parametrize("name", sorted(PINNED))
def test_replan_end_to_end(engine, name):
    """search(...).replan(...) for the corridor scenarios of tests/test_replan.py: FOUND at the bits of the cost of
    EnvMap.search(root_state, goal, start_g=g_root) on the edited map, with the model's kept nodes, bad edges, rounds and
    expansions; the path rolls out complete on the edited map at cost - g_root (edge costs 10, 10.25, 10.5: exact sums)."""
    m = engine
    w, sc = world(m), SCENARIOS[name]
    n0, kept, bad, cost, rounds, expanded, f_rounds, f_expanded = PINNED[name]
    env, start, _ = corridor_env(m, w.map_of(sc["first"]))
    goal0, goal = w.goal, w.goal_of(sc)
    cap = sc.get("cap", 1 << 15)
    r0 = env.search(start, goal0, eps=EPS, delta=DELTA, capacity=1 << 15, max_frontier=cap if "cap" in sc else None, sight=False)
    assert r0.found and r0.table.stats()[0] == n0
    ids, _ = r0.table.path(r0.goal_id)
    root = int(ids[sc["advance"]])
    d0 = r0.table.download()
    g_root, s_root = float(d0["g"][root]), d0["state"][:, root].copy()
    new = w.cells(sc["wall"])
    changed = np.nonzero(new != w.map_of(sc["first"]))[0]
    if changed.size:
        env.editMap(changed, new[changed])
    r1 = r0.replan(advance=sc["advance"] if sc["advance"] else None, goal_row=goal if "goal" in sc else None)
    assert r0.table is None and r1.table is not None
    print(name, r1, r1.rebase_info)
    assert r1.found and bits([r1.cost])[0] == bits([cost])[0]
    assert (r1.rebase_info["n_kept"], r1.rebase_info["n_bad_edges"], r1.rounds, r1.expanded) == (kept, bad, rounds, expanded)
    fresh = env.search(s_root, goal, eps=EPS, delta=DELTA, capacity=1 << 15, sight=False, start_g=g_root)
    assert fresh.found and bits([fresh.cost])[0] == bits([r1.cost])[0] and (fresh.rounds, fresh.expanded) == (f_rounds, f_expanded)
    fresh.free()
    assert bits([rollout_cost(m, env, r1)])[0] == bits([r1.cost - g_root])[0]
    start_state, _ = r1.path()
    assert np.array_equal(bits(start_state), bits(s_root))
    if sc["wall"] is not None:
        # a second replan on the returned result: the wall goes, and the cost from the original start is 351.5 again
        env.editMap(changed, w.grid[changed])
        r2 = r1.replan()
        assert r1.table is None and r2.found and r2.cost == 351.5 and r2.rebase_info["n_bad_edges"] == 0
        assert bits([rollout_cost(m, env, r2)])[0] == bits([351.5 - g_root])[0]
        r2.free()
    else:
        r1.free()
    with pytest.raises(RuntimeError):
        r0.replan()
    env.close()


def test_replan_many_end_to_end(engine):
    """search_many(...).replan(advance=5) for three queries with the wall across q0's middle edge: every query FOUND at
    the cost of its own fresh search from its root on the edited map."""
    m = engine
    w = world(m)
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    r0 = env.search_many(starts, goals, eps=EPS, delta=DELTA, capacity=1 << 16, sight=False)
    d0 = r0.table.download()
    roots = [int(r0.table.path(r0.goal_id[q])[0][5]) for q in range(3)]
    g_root, s_root = d0["g"][roots], d0["state"][:, roots].copy()
    env.editMap(w.walls["mid"], 100)
    r1 = r0.replan(advance=5)
    print(r1, r1.rebase_info, r1.cost)
    assert r0.table is None and all(r1.found) and r1.rebase_info["n_roots"] == 3 and r1.rebase_info["n_bad_edges"] >= 1
    fresh = env.search_many(s_root, goals, eps=EPS, delta=DELTA, capacity=1 << 16, sight=False, start_g=g_root)
    assert all(fresh.found)
    for q in range(3):
        assert bits([r1.cost[q]])[0] == bits([fresh.cost[q]])[0], q
        one = env.search(s_root[:, q], goals[q], eps=EPS, delta=DELTA, capacity=1 << 15, sight=False, start_g=float(g_root[q]))
        assert bits([one.cost])[0] == bits([r1.cost[q]])[0], q
        one.free()
        start_state, act = r1.path(q)
        out = env.rollout(start_state, act.reshape(-1, 1))
        assert out["status"][0] == m.SLOT_FINITE and bits(out["cost"])[0] == bits([r1.cost[q] - g_root[q]])[0], q
    assert r1.total_rounds < fresh.total_rounds and sum(r1.expanded) >= r1.rebase_info["n_kept"]
    # and again on the returned result: without the wall q0 costs 351.5 once more
    env.editMap(w.walls["mid"], w.grid[w.walls["mid"]])
    r2 = r1.replan()
    assert all(r2.found) and r2.cost == [351.5, 351.75, 352.0]
    fresh.free()
    r2.free()
    env.close()


# ---- 6. yaw controls: heading-limit decisions inside the band of the yaw pinning count as bad
YAW_GOAL = (0.75, -1.25)  # from the start; reachable under the heading limit (three edges on the unedited map)


def yaw_world(m, control=0x13, live=False):
    wl = _small_world(m, 2, control, seed=5, edge=32)
    start = small_start(wl)
    if live:
        start = np.array(CM.live_start(start, 2, control))
    goal = np.zeros(10)
    goal[:2] = start[:2] + YAW_GOAL
    return wl, start, goal


def test_yaw_controls(engine, oracle_lib):
    yaw_controls(engine, oracle_lib, 0x13, False)


def test_yaw_controls_jrk(engine, oracle_lib):
    """The JRKxYAW twin, from a live acc row: replan_edge_kernel<2, 3, true, false>."""
    yaw_controls(engine, oracle_lib, 0x17, True)


def yaw_controls(m, O, control, live):
    wl, start, goal = yaw_world(m, control, live)
    far = np.zeros(10)
    far[:2] = start[:2] + [1.2, -0.8]  # (the goal of test_four_rounds_with_yaw_controls: not reached in four rounds)
    env = engine_env(m, wl)
    r = env.search(start, far, eps=1.0, delta=2.0, max_rounds=4, capacity=1 << 14, tol_pos=wl.res)
    tab = r.table
    d0 = tab.download()
    assert d0["n_nodes"] > 30
    t0 = RM.table_from_arrays(d0)
    dep = depths(t0)
    cells = sorted(set(cell_index(wl.map_dim, wl.origin, wl.res, t0.state[i]) for i in range(t0.n_nodes) if dep[i] == 2))[::3][:6]
    grid = np.array(wl.grid, dtype=np.int8).ravel().copy()
    grid[cells] = 100
    env.editMap(cells, 100)
    model = RM.table_from_arrays(d0)
    want_fr, want, _ = RM.rebase(model, RM.OracleEdges(O, oracle_env_with(O, wl, grid), model), len(wl.U), root=-1)
    assert want["n_bad_edges"] >= 1 and want["n_kept"] >= 2
    fr = m.TableFrontier(env, d0["n_nodes"])
    got = tab.rebase(root=-1, frontier=fr)
    d1 = tab.download()
    dropped_dev, dropped_model = ~np.isfinite(d1["g"]), ~np.isfinite(np.array(model.g))
    assert not (dropped_model & ~dropped_dev).any()  # the device's bad set contains the model's
    assert got["n_roots"] == want["n_roots"] == 1 and got["n_kept"] <= want["n_kept"]
    # a node the device dropped below a parent it kept, and the model keeps: its own edge was bad on the device alone --
    # the pair (parent, action) must carry MPLX_ROLLOUT_HEADING_BAND at horizon 1
    extra = [i for i in range(d0["n_nodes"]) if dropped_dev[i] and not dropped_model[i] and d0["pred"][i] >= 0 and
             not dropped_dev[d0["pred"][i]]]
    if extra:
        st = np.ascontiguousarray(d0["state"][:, d0["pred"][extra]])
        a = np.ascontiguousarray(d0["pred_action"][extra].astype(np.int32))
        sd, ad = m.DeviceArray(env, st.nbytes), m.DeviceArray(env, a.nbytes)
        sd.upload(st)
        ad.upload(a)
        out = env.alloc_rollouts(len(extra), want_end=False)
        env.rollout_resident(sd, ad, out, 1)
        env.synchronize()
        assert np.all(out.download()["status"] & m._abi.ROLLOUT_HEADING_BAND), extra
        for b in (sd, ad, out):
            b.free()
    else:
        assert got == want and np.array_equal(fr.download()["id"], want_fr["id"])
    fr.free()
    r.free()
    # the replan's cost is the fresh search's
    env.editMap(cells, np.array(wl.grid, dtype=np.int8).ravel()[cells])
    r0 = env.search(start, goal, eps=1.0, delta=2.0, capacity=1 << 14, tol_pos=wl.res)
    assert r0.found
    ids, _ = r0.table.path(r0.goal_id)
    s1 = r0.table.state_of(int(ids[1]))
    cell = cell_index(wl.map_dim, wl.origin, wl.res, s1)
    env.editMap([cell], 100)
    r1 = r0.replan()
    fresh = env.search(start, goal, eps=1.0, delta=2.0, capacity=1 << 14, tol_pos=wl.res)
    print(r0, r1, fresh, r1.rebase_info)
    assert r1.status == fresh.status and r1.rebase_info["n_bad_edges"] >= 1
    assert bits([r1.cost])[0] == bits([fresh.cost])[0]
    fresh.free()
    r1.free()
    env.close()


# ---- 7. errors and state
def test_argument_errors_and_state(engine):
    m = engine
    L_ = m._abi.lib()
    OK, ARG, STATE = m._abi.OK, m._abi.ERR_ARG, m._abi.ERR_STATE
    env = rest_env(m)  # parameters and controls, no map
    tab = env.alloc_table(64)
    opn = env.alloc_open(tab)
    fr = patterned_frontier(m, env, 8, 8)
    res = m._abi.RebaseResult()

    def rebase(t=tab._tab, root=-1, check=0, f=None, h=True):
        f = fr.c_struct() if f is None else f
        return L_.mplx_table_rebase_device(t, root, check, C.byref(f), None, C.byref(res) if h else None)
    assert rebase(t=None) == ARG and rebase(root=-2) == ARG
    assert L_.mplx_table_rebase_device(tab._tab, -1, 0, None, None, None) == ARG
    assert L_.mplx_table_rebase_multi_device(tab._tab, None, 0, C.byref(fr.c_struct()), None, None) == ARG
    assert L_.mplx_table_rebase_multi_device(None, None, 0, None, None, None) == ARG
    assert L_.mplx_open_push_closed_device(None, C.byref(fr.c_struct()), 1, 1.0, 0) == ARG
    assert L_.mplx_open_push_closed_device(opn._open, None, 1, 1.0, 0) == ARG
    for field, v in (("id", None), ("g", None), ("state", None), ("count", None), ("state_stride", 7), ("capacity", -1)):
        f = fr.c_struct()
        setattr(f, field, v)
        assert rebase(f=f) == ARG, field
    assert rebase(check=1) == STATE  # no map
    assert L_.mplx_open_push_closed_device(opn._open, C.byref(fr.c_struct()), 1, 1.0, 0) == STATE  # no goal
    # an empty table: a successful no-op with count 0 and nothing written
    fr.count.upload(np.array([77], np.int64))
    assert rebase() == OK and (res.n_kept, res.n_bad_edges, res.n_roots) == (0, 0, 0)
    assert int(fr.count.download(np.int64, (1,))[0]) == 0
    assert tab.rebase(root=5, check_edges=False, frontier=fr) == {"n_kept": 0, "n_bad_edges": 0, "n_roots": 0}
    assert_spare_untouched(fr)
    # seeds only, every kind of root; a root that is none keeps nothing
    states = np.zeros((10, 3))
    states[0] = [0.0, 0.5, 1.0]
    imp = m.TableFrontier(env, 8)
    assert tab.seed(states, g=[0.0, 1.5, 2.0], frontier=imp) == 3
    assert tab.rebase(root=-1, check_edges=False, frontier=fr) == {"n_kept": 3, "n_bad_edges": 0, "n_roots": 3}
    assert tab.rebase(root=1, check_edges=False, frontier=fr) == {"n_kept": 1, "n_bad_edges": 0, "n_roots": 1}
    got = fr.download()
    assert got["id"].tolist() == [1] and got["g"].tolist() == [1.5]
    assert tab.rebase(root=0, check_edges=False, frontier=fr)["n_kept"] == 0  # node 0 was dropped: g = +inf, no root
    for root in (3, 63, 64, 2 ** 31 - 1):
        assert tab.rebase(root=root, check_edges=False, frontier=fr)["n_kept"] == 0, root
    assert np.all(np.isinf(tab.download()["g"]))
    assert tab.rebase(roots=[1], check_edges=False, frontier=fr)["n_kept"] == 0  # the _multi call takes a table of one query
    env.set_goal(np.zeros(10))
    opn.push(imp, n_max=3, eps=1.0, closed=True)
    assert np.array_equal(opn.download()["flags"] & m.search.IS_OPEN, np.zeros(3, np.uint8))
    # a status bit on the table
    from test_gpu_table import distinct_list, upload, upload_lists
    lists = upload_lists(m, env, distinct_list(np.random.default_rng(3), 40))
    pid, pg = upload(env, m, np.zeros(1, np.int32)), upload(env, m, np.zeros(1))
    small = env.alloc_table(8)
    big = m.TableFrontier(env, 64)
    small.relax(lists, pid, pg, frontier=big, want_count=False)
    assert small.rebase(root=-1, check_edges=False, frontier=big, want_result=False) is None  # queued before the host saw the bit
    assert small.stats()[1] & m.table.NODES_FULL
    with pytest.raises(m._abi.MplxError) as err:
        small.rebase(root=-1, check_edges=False, frontier=big)
    assert err.value.code == STATE
    for b in (fr, imp, lists, pid, pg, big):
        b.free()
    small.free()
    opn.free()
    tab.free()
    env.close()


def test_replan_of_a_result_whose_table_has_a_status_bit(engine):
    m = engine
    env, start, goal = corridor_env(m)
    r = env.search(start, goal, eps=EPS, delta=DELTA, max_rounds=3, capacity=1 << 12, sight=False)
    assert r.status == m.search.MAX_ROUNDS
    # the table's capacity is also the kept frontier's: a relax that overflows the node array sets the bit
    lists = env.alloc_lists(1 << 12, want_state=True)
    sel, imp = m.TableFrontier(env, 1 << 12), m.TableFrontier(env, 1 << 12)
    for _ in range(40):
        got = r.open.select(math.inf, sel)
        if got["status"] != m.search.SELECTED:
            break
        env.expand_lists_resident(sel, lists, n_nodes=got["count"])
        r.table.relax(lists, sel.id, sel.g, frontier=imp, n_nodes=got["count"], want_count=False)
        r.open.push(imp, n_max=got["count"] * lists.stride, eps=EPS)
        if r.table.stats()[1]:
            break
    assert r.table.stats()[1] & m.table.NODES_FULL
    with pytest.raises(m._abi.MplxError) as err:
        r.replan()
    assert err.value.code == m._abi.ERR_STATE and r.table is not None  # the old result still owns its table
    for b in (lists, sel, imp):
        b.free()
    r.free()
    env.close()
