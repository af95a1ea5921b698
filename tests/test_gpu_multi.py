"""GPU: Q queries in one node table and one open set (include/mplx_multi.h) against tests/multi_model.py, bit for bit as
tests/test_gpu_table.py and tests/test_gpu_open.py compare: node arrays with the query column, every frontier row, f and
flags of every node and the Q results of every select.  tests/test_multi.py shows on the CPU that the batch model is Q
single models under the renumbering; test_separation_* shows the same of the device against EnvMap.search itself."""
import ctypes as C
import math

import numpy as np
import pytest

import control_matrix as CM
import multi_model as MM
import open_model as OM
from helpers import engine_env, oracle_env
from table_model import EMPTY, F2, TableModel, oracle_provider
from test_gpu_open import (assert_open_equal, assert_result_equal, assert_spare_untouched, corridor_env, patterned_frontier,
                           rest_env, small_world_goal, upload_frontier, _goals)
from test_gpu_parity import _small_world
from test_gpu_table import assert_frontier_equal, assert_table_equal, bits, distinct_list, upload, upload_lists
from test_multi import corridor_queries, hand_models
from test_table import small_start

pytestmark = pytest.mark.gpu


def assert_multi_table_equal(tab, model, what=""):
    got = assert_table_equal(tab, model, what)
    assert np.array_equal(got["query"], np.asarray(model.query, dtype=np.int32)), what + ": query"
    return got


def select_many_both(opn, model, delta, fr, what="", d_results=None):
    got = opn.select_many(delta, fr, d_results=d_results)
    want, want_fr = model.select_many(delta, fr.capacity)
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert_result_equal(g, w, "%s: query %d" % (what, q))
    assert_frontier_equal(fr.download(), want_fr, what)
    assert sum(g["count"] for g in got) == want_fr["count"]
    return got, want_fr


def relax_both(m, env, tab, model, host, parent_id, parent_g, fr, g_max=math.inf):
    """One relax on the device (into `fr`, which stays) and in the model: frontier and entry ids compared."""
    n, S = len(host["count"]), int(host["stride"])
    L = upload_lists(m, env, host)
    d_pid, d_pg = upload(env, m, parent_id.astype(np.int32)), upload(env, m, parent_g.astype(np.float64))
    d_eid = upload(env, m, np.full(n * S, -7, np.int32))
    cnt = tab.relax(L, d_pid, d_pg, g_max, frontier=fr, entry_id=d_eid)
    want_fr, want_eid = model.relax(host, parent_id, parent_g, g_max)
    assert np.array_equal(d_eid.download(np.int32, (n * S,)), want_eid)
    assert_frontier_equal(fr.download(cnt), want_fr)
    for b in (d_pid, d_pg, d_eid, L):
        b.free()
    return want_fr, want_eid


def test_hand_built_relax_push_and_select(engine, oracle_lib):
    """tests/multi_model.py::hand_seeds / hand_relax (their properties: tests/test_multi.py), Q = 3: the same hash in two
    queries is two nodes, the hash equal to the empty marker lives in several queries, rows whose parent is no node of
    the table touch nothing, equal candidates inside a query, find per query, selects with and without a cut."""
    m = engine
    table, model, states, query, g, goals, hashes = hand_models()
    env = rest_env(m)
    tab = env.alloc_table(4096, n_queries=MM.HAND_Q)
    opn = env.alloc_open(tab)
    opn.set_goals(goals, tol_pos=MM.HAND_TOL)
    imp = m.TableFrontier(env, 1024)
    cnt = tab.seed(states, g, frontier=imp, query=query)
    want_imp, _ = table.seed(states, hashes, g, query)
    assert cnt == 42 == table.n_nodes
    assert_frontier_equal(imp.download(cnt), want_imp, "seed")
    assert_multi_table_equal(tab, table, "seed")
    opn.push(imp, n_max=cnt, eps=1.0)
    model.push(want_imp, cnt, 1.0)
    assert_open_equal(opn, model, "push of the seeds")
    big, cut = patterned_frontier(m, env, 2048, 64), patterned_frontier(m, env, 8, 64)
    d_res = m.DeviceArray(env, 48 * MM.HAND_Q + 64)
    d_res.upload(np.full(48 * MM.HAND_Q + 64, 0xA5, np.uint8))
    got, _ = select_many_both(opn, model, 0.0, big, "select 0", d_results=d_res)
    raw = d_res.download(np.uint8, (48 * MM.HAND_Q + 64,))
    assert np.all(raw[48 * MM.HAND_Q:] == 0xA5)  # Q results, nothing behind them
    for q in range(MM.HAND_Q):
        r = m._abi.OpenResult.from_buffer_copy(raw[48 * q:48 * (q + 1)].tobytes())
        assert (r.status, r.goal_id, r.count, r.n_open) == (got[q]["status"], got[q]["goal_id"], got[q]["count"], got[q]["n_open"])
        assert bits([r.f_min, r.goal_f, r.goal_g]).tolist() == bits([got[q]["f_min"], got[q]["goal_f"], got[q]["goal_g"]]).tolist()
    assert_open_equal(opn, model, "select 0")
    rng = np.random.default_rng(17)
    statuses = set()
    for call in range(2):
        n_before = table.n_nodes
        lists, pid, pg, pool = MM.hand_relax(rng, n_before)
        want_imp, want_eid = relax_both(m, env, tab, table, lists, pid, pg, imp)
        S = lists["stride"]
        for k in (5, 11, 17, 23):  # parents -1, n_before, n_before + 5, 2^31 - 1
            assert np.all(want_eid[k * S:(k + 1) * S] == -1)
        assert_multi_table_equal(tab, table, "relax %d" % call)
        opn.push(imp, n_max=len(pid) * S, eps=1.0)
        model.push(want_imp, len(pid) * S, 1.0)
        assert_open_equal(opn, model, "push %d" % call)
        for delta, fr in ((0.5, cut), (0.5, big), (math.inf, cut), (math.inf, big)):
            what = "select %d (%r, %d)" % (call, delta, fr.capacity)
            got, _ = select_many_both(opn, model, delta, fr, what)
            statuses |= {r["status"] for r in got}
            assert_spare_untouched(fr, what)
            assert_open_equal(opn, model, what)
    assert {OM.SELECTED, OM.FOUND} <= statuses
    a = table.arrays()
    assert sum(1 for k in table.ids if k[1] == int(EMPTY)) >= 2
    # find: every node by (query, hash); a hash that only another query holds; a stranger; the plain calls refuse
    assert np.array_equal(tab.find(a["hash"], a["query"]), np.arange(a["n_nodes"], dtype=np.int32))
    only0 = [h for q, h in table.ids if q == 0 and (1, h) not in table.ids]
    assert only0 and np.all(tab.find(only0, 1) == -1) and tab.find([12345], 2)[0] == -1
    d_h, d_q = upload(env, m, a["hash"]), upload(env, m, np.where(np.arange(a["n_nodes"]) % 5 == 0, 7, a["query"]).astype(np.int32))
    d_id = m.DeviceArray(env, a["n_nodes"] * 4)
    assert m._abi.lib().mplx_table_find_multi_device(tab._tab, d_h.ptr, d_q.ptr, a["n_nodes"], d_id.ptr) == m._abi.OK
    want = np.where(np.arange(a["n_nodes"]) % 5 == 0, -1, np.arange(a["n_nodes"])).astype(np.int32)  # query 7: no such query
    assert np.array_equal(d_id.download(np.int32, (a["n_nodes"],)), want)
    for b in (imp, big, cut, d_res, d_h, d_q, d_id):
        b.free()
    opn.free()
    tab.free()
    env.close()


def device_search_many(m, env, table, model, starts, hashes, eps, delta, cap, g_max, sight, max_rounds, capacity=1 << 15,
                       stop=None, slots_log2=0):
    """The loop of EnvMap.search_many spelled out, every step compared with the model fed with the device's own lists.
    Returns (table, open set, the last results, rounds, the result of every select [round][Q])."""
    Q = starts.shape[1]
    tab = env.alloc_table(capacity, slots_log2, n_queries=Q)
    opn = env.alloc_open(tab)
    opn.set_goals(model.goals, w=model.w, v_max=model.v_max, tol_pos=model.tol[0])
    sel, imp = patterned_frontier(m, env, cap, 32), m.TableFrontier(env, capacity)
    lists = env.alloc_lists(cap, want_state=True)
    count = tab.seed(starts, frontier=imp, query=np.arange(Q, dtype=np.int32))
    want_imp, _ = table.seed(starts, hashes, query=np.arange(Q))
    assert_frontier_equal(imp.download(count), want_imp, "seed")
    opn.push(imp, n_max=count, eps=eps, sight=sight)
    model.push(want_imp, count, eps, sight)
    rounds, history = 0, []
    while True:
        what = "round %d" % rounds
        assert_open_equal(opn, model, what)
        got, want_sel = select_many_both(opn, model, delta, sel, what)
        history.append(got)
        n = want_sel["count"]
        if not any(r["status"] == OM.SELECTED for r in got) or rounds >= max_rounds or (stop and stop(table, rounds)):
            break
        env.expand_lists_resident(sel, lists, n_nodes=n)
        cnt = tab.relax(lists, sel.id, sel.g, g_max, frontier=imp, n_nodes=n)
        want_imp, _ = table.relax(lists.download_nodes(0, n), want_sel["id"], want_sel["g"], g_max)
        assert_frontier_equal(imp.download(cnt), want_imp, what + ": relax")
        opn.push(imp, n_max=n * lists.stride, eps=eps, sight=sight)
        model.push(want_imp, n * lists.stride, eps, sight)
        rounds += 1
    assert_spare_untouched(sel)
    assert_multi_table_equal(tab, table, "the end")
    for b in (sel, imp, lists):
        b.free()
    return tab, opn, got, rounds, history


def world_model(O, wl, dim, control, env, starts, goals, tol):
    Q = starts.shape[1]
    table = MM.MultiTableModel(4 * dim + 2, Q)
    model = MM.MultiOpenModel(table, dim, goals, [O.lattice_hash(dim, control, g) for g in goals], env._p.w, env._p.v_max, tol_pos=tol,
                              blocked=[OM.ray_blocked(wl.grid, wl.map_dim, wl.origin, wl.res, g[:dim]) for g in goals])
    return table, model, [O.lattice_hash(dim, control, starts[:, q]) for q in range(Q)]


def wall_in(wl, pos):
    """Occupies the cell of `pos` and every cell within two cells of it (the tolerance box of one cell and its rim)."""
    md = wl.map_dim
    grid = np.array(wl.grid, dtype=np.int8).reshape(md[::-1]).copy()
    cell = np.floor((np.asarray(pos) - np.asarray(wl.origin)) / wl.res).astype(int)
    sl = tuple(slice(max(c - 2, 0), c + 3) for c in cell[::-1])
    grid[sl] = 100
    wl.grid = np.ascontiguousarray(grid.ravel())


WORLDS = {(2, 0x03, 56.0, 32), (3, 0x07, 46.0, 64)}


# 2D SNP from live acc and jerk rows (tests/control_matrix.py) -> per third query: the statuses and total rounds of
# tests/multi_model.py on the oracle's lists
SNP_MODEL = {"inside": ([OM.FOUND, OM.FOUND, OM.FOUND], 4), "walled": ([OM.FOUND, OM.FOUND, OM.EMPTY], 11)}


@pytest.mark.parametrize("third", ["inside", "walled"])
@pytest.mark.parametrize("world", sorted(WORLDS) + [pytest.param(CM.SNP_WORLD, id="2d-snp")])
def test_search_round_by_round(engine, oracle_lib, world, third):
    """2D ACC, 3D JRK and 2D SNP, Q = 3, with the ray trace, every round compared.  Queries 0 and 1 cross (q0's start is q1's
    goal and the other way round).  Query 2 either starts inside its own goal region -- FOUND at the first select and
    the same result in every later round -- or aims at a goal that is walled in: EMPTY while the others go on."""
    m, O = engine, oracle_lib
    dim, control, g_max, edge = world
    if world not in _goals:
        _goals[world] = small_world_goal(m, O, dim, control, g_max, edge)
    _, start, h0, goal = _goals[world]
    wl = _small_world(m, dim, control, seed=5, edge=edge)
    back = np.zeros(4 * dim + 2)
    back[:dim] = goal[:dim]  # at rest at q0's goal
    starts = np.stack([start, back, start], axis=1)
    goals = np.stack([goal, start, start])
    if third == "walled":
        free = np.argwhere(np.asarray(wl.grid).reshape(wl.map_dim[::-1]) == 0)[:, ::-1]
        far = free[np.argmax(np.minimum(np.abs(free - (start[:dim] / wl.res)).max(axis=1), np.abs(free - (goal[:dim] / wl.res)).max(axis=1)))]
        goals[2, :dim] = np.asarray(wl.origin) + (far + 0.5) * wl.res
        wall_in(wl, goals[2, :dim])
    env = engine_env(m, wl)
    table, model, hashes = world_model(O, wl, dim, control, env, starts, goals, wl.res)
    if world not in WORLDS:  # the pinned numbers are the model's on the oracle: held before the device runs
        t2, m2, _ = world_model(O, wl, dim, control, env, starts, goals, wl.res)
        out = MM.search_many(t2, m2, oracle_provider(O, oracle_env(wl)), starts, hashes, 1.0, 5.0, 8192, g_max, True)
        closed = sum(1 for fl in m2.flags.values() if fl & OM.SEEN and not fl & OM.IS_OPEN)
        print("model on the oracle:", world, third, out["status"], out["total_rounds"], "closed", closed, "nodes", t2.n_nodes)
        assert (out["status"], out["total_rounds"]) == SNP_MODEL[third] and out["total_rounds"] >= 3
        assert closed >= 1 and 100 <= t2.n_nodes <= 20000
    tab, opn, got, rounds, history = device_search_many(m, env, table, model, starts, hashes, 1.0, 5.0, 8192, g_max, True, 10 ** 6)
    print(world, third, rounds, [r["status"] for r in got], table.n_nodes)
    if world not in WORLDS:
        assert ([r["status"] for r in got], rounds) == SNP_MODEL[third]
    # (the way back ends at rest at q0's start: within g_max the 2D ACC world reaches it, the 3D JRK world does not; in
    # the 2D SNP world it does)
    assert got[0]["status"] == OM.FOUND and got[1]["status"] == (OM.FOUND if dim == 2 else OM.EMPTY) and rounds >= 3
    if third == "inside":
        assert all(h[2]["status"] == OM.FOUND and h[2] == history[0][2] for h in history)
        assert history[0][2]["goal_g"] == 0.0 and history[0][2]["count"] == 0
    else:
        first_empty = [k for k, h in enumerate(history) if h[2]["status"] == OM.EMPTY]
        assert got[2]["status"] == OM.EMPTY and got[2]["goal_id"] == -1 and history[0][2]["status"] == OM.SELECTED
        assert all(h[2] == got[2] for h in history[first_empty[0]:])
    # the chains of best predecessors stay inside their query
    a = table.arrays()
    for q in (0, 1):
        if got[q]["status"] != OM.FOUND:
            continue
        ids, act = tab.path(got[q]["goal_id"])
        assert np.all(a["query"][ids] == q) and a["pred"][ids[0]] == -1 and len(act) >= 3
    opn.free()
    tab.free()
    env.close()


def renumbered_device(res, q):
    tab = res.table.download()
    opn = res.open.download()
    return MM.restrict(tab, q, opn["f"], opn["flags"])


def assert_query_is_single(multi, q, single, what=""):
    """Query q of a search_many result against an EnvMap.search result, under the renumbering, bit for bit."""
    sub, f, fl, rank = renumbered_device(multi, q)
    want, wopn = single.table.download(), single.open.download()
    assert sub["n_nodes"] == want["n_nodes"], what
    for k in ("hash", "pred", "pred_action"):
        assert np.array_equal(sub[k], want[k]), "%s: %s" % (what, k)
    assert np.array_equal(bits(sub["g"]), bits(want["g"])) and np.array_equal(bits(sub["state"]), bits(want["state"])), what
    assert np.array_equal(fl, wopn["flags"]), what
    seen = (fl & OM.SEEN) > 0
    assert np.array_equal(bits(f[seen]), bits(wopn["f"][seen])), what
    assert multi.status[q] == single.status and (multi.rounds[q], multi.expanded[q]) == (single.rounds, single.expanded), what
    assert_result_equal(MM.renumber_result(multi.last_select[q], rank), single.last_select, what)
    assert bits([multi.cost[q]])[0] == bits([single.cost])[0]
    if single.found:
        (s1, a1), (s2, a2) = multi.path(q), single.path()
        assert np.array_equal(bits(s1), bits(s2)) and np.array_equal(a1, a2), what
    return sub


def test_twin_queries(engine, oracle_lib):
    """Queries 0 and 1 have the same start and goal: both equal the single search, on disjoint nodes."""
    m, O = engine, oracle_lib
    world = (2, 0x03, 56.0, 32)
    if world not in _goals:
        _goals[world] = small_world_goal(m, O, *world)
    wl, start, h0, goal = _goals[world]
    env = engine_env(m, wl)
    kw = dict(eps=1.0, delta=5.0, g_max=56.0, capacity=1 << 15, tol_pos=wl.res)
    single = env.search(start, goal, **kw)
    multi = env.search_many(np.stack([start, start], axis=1), np.stack([goal, goal]), **kw)
    assert single.found and multi.found == [True, True]
    for q in (0, 1):
        assert_query_is_single(multi, q, single, "twin %d" % q)
    tab = multi.table.download()
    assert tab["n_nodes"] == 2 * single.table.stats()[0] and sorted(tab["query"].tolist()) == [0] * (tab["n_nodes"] // 2) + [1] * (tab["n_nodes"] // 2)
    assert multi.goal_id[0] != multi.goal_id[1]
    single.free()
    multi.free()
    env.close()


@pytest.mark.parametrize("delta", [0.0, 10.0])
def test_separation_on_the_corridor(engine, delta):
    """EnvMap.search_many on the corridor of test_planner_2d (its own query, a shifted one, the way back; the ray trace
    on) against three EnvMap.search runs in the same process: no selection is cut, so every query is its single search
    under the renumbering.  The published cost, and paths a rollout accepts."""
    m = engine
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    kw = dict(eps=1.0, delta=delta, capacity=1 << 16)
    multi = env.search_many(starts, goals, **kw)
    print(multi, multi.rounds, multi.expanded)
    assert multi.found == [True] * 3 and multi.cost[0] == 351.5
    for q in range(3):
        single = env.search(starts[:, q], goals[q], **kw)
        assert_query_is_single(multi, q, single, "query %d" % q)
        single.free()
        s0, act = multi.path(q)
        r = env.rollout(s0, act.reshape(-1, 1))
        assert r["status"][0] == m.SLOT_FINITE and r["steps"][0] == len(act) and bits(r["cost"])[0] == bits([multi.cost[q]])[0]
    assert len(multi.path(0)[1]) == 35 and multi.total_rounds == max(multi.rounds)
    multi.free()
    env.close()


def test_more_queries_than_lanes(engine, oracle_lib):
    """Q = 70 on the small 2D world: a wave of the select holds several queries, the query index exceeds a wave, and the
    table grows past 4 096 nodes, so tiles and per-query decisions cross tile boundaries.  Every round compared."""
    m, O = engine, oracle_lib
    wl = _small_world(m, 2, 0x03, seed=5, edge=32)
    free = np.argwhere(np.asarray(wl.grid).reshape(wl.map_dim[::-1]) == 0)[:, ::-1]
    rng = np.random.default_rng(70)
    pick = free[rng.choice(len(free), 140, replace=False)]
    pos = np.asarray(wl.origin) + (pick + 0.5) * wl.res
    Q = 70
    starts, goals = np.zeros((10, Q)), np.zeros((Q, 10))
    starts[:2], goals[:, :2] = pos[:Q].T, pos[Q:]
    goals[5, :2] = starts[:2, 5]  # one query is done at once
    env = engine_env(m, wl)
    table, model, hashes = world_model(O, wl, 2, 0x03, env, starts, goals, wl.res)
    big = {"rounds": None}

    def stop(t, rounds):  # two more rounds once the table has passed a tile
        if big["rounds"] is None and t.n_nodes > 4096:
            big["rounds"] = rounds
        return big["rounds"] is not None and rounds >= big["rounds"] + 2
    tab, opn, got, rounds, history = device_search_many(m, env, table, model, starts, hashes, 1.0, 5.0, 8192, math.inf, True, 12,
                                                        capacity=1 << 16, stop=stop)
    print(rounds, table.n_nodes, sorted(set(r["status"] for r in got)))
    assert table.n_nodes > 4096 and big["rounds"] is not None
    a = table.arrays()
    assert len(set(a["query"].tolist())) == Q and history[0][5]["status"] == OM.FOUND
    runs = np.count_nonzero(np.diff(a["query"][:4096].astype(np.int64)))  # the queries are interleaved inside the waves
    assert runs > 100
    opn.free()
    tab.free()
    env.close()


def test_four_rounds_with_yaw_controls(engine, oracle_lib):
    four_rounds_with_yaw(engine, oracle_lib, 0x13)


def test_four_rounds_with_jrk_yaw_controls(engine, oracle_lib):
    """The JRKxYAW twin, from a live acc row."""
    four_rounds_with_yaw(engine, oracle_lib, 0x17, live=True)


def four_rounds_with_yaw(m, O, control, live=False):
    wl = _small_world(m, 2, control, seed=5, edge=32)
    start = small_start(wl)
    if live:
        start = np.array(CM.live_start(start, 2, control))
    starts = np.stack([start, start], axis=1)
    goals = np.zeros((2, 10))
    goals[0, :2] = start[:2] + [1.2, -0.8]
    goals[1, :2] = start[:2] + [-0.9, 0.7]
    env = engine_env(m, wl)
    table, model, hashes = world_model(O, wl, 2, control, env, starts, goals, wl.res)
    tab, opn, got, rounds, _ = device_search_many(m, env, table, model, starts, hashes, 1.0, 2.0, 8192, math.inf, True, 4)
    assert rounds == 4 and table.n_nodes > 60 and [r["status"] for r in got] == [OM.SELECTED] * 2
    opn.free()
    tab.free()
    env.close()


def test_capacity_cut(engine, oracle_lib):
    """A frontier of 8 rows under Q = 3: every selection is cut in global id order; every row equals the model, the
    spare rows are untouched, and the costs are those of the uncut run."""
    m, O = engine, oracle_lib
    world = (2, 0x03, 56.0, 32)
    if world not in _goals:
        _goals[world] = small_world_goal(m, O, *world)
    wl, start, h0, goal = _goals[world]
    back = np.zeros(10)
    back[:2] = goal[:2]
    near = np.zeros(10)
    near[:2] = start[:2] + [0.5, 0.3]  # (a free cell: query 2 is done early and sits still while the others are cut)
    starts, goals = np.stack([start, back, start], axis=1), np.stack([goal, start, near])
    env = engine_env(m, wl)
    table, model, hashes = world_model(O, wl, 2, 0x03, env, starts, goals, wl.res)
    tab, opn, got, rounds, history = device_search_many(m, env, table, model, starts, hashes, 1.0, 5.0, 8, 56.0, True, 10 ** 6)
    cuts = sum(1 for h in history if sum(r["count"] for r in h) == 8 and any(r["status"] == OM.SELECTED and r["n_open"] > 0 for r in h))
    uncut = env.search_many(starts, goals, eps=1.0, delta=5.0, g_max=56.0, capacity=1 << 15, tol_pos=wl.res)
    print(rounds, cuts, [r["status"] for r in got], uncut)
    assert cuts > 10 and [r["status"] for r in got] == uncut.status == [OM.FOUND] * 3
    assert bits([r["goal_g"] for r in got]).tolist() == bits(uncut.cost).tolist()
    uncut.free()
    opn.free()
    tab.free()
    env.close()


def test_full_regions(engine, oracle_lib):
    """Regions of 16 slots in a table of 256 nodes: 16 keys of one query just fit (long probe chains inside the region,
    equal to the model); the 17th raises PROBE_FULL | NODES_FULL although the node arrays have room, the bits stick,
    later calls are MPLX_ERR_STATE and nothing is written behind a frontier's capacity."""
    m, O = engine, oracle_lib
    env = rest_env(m)
    rng = np.random.default_rng(8)
    seeds = np.zeros((F2, 2))
    seeds[0] = [0.3, 0.7]
    hashes = [O.lattice_hash(2, O.ACC, seeds[:, k]) for k in range(2)]
    tab = env.alloc_table(256, slots_log2=4, n_queries=2)
    table = MM.MultiTableModel(F2, 2)
    fr = patterned_frontier(m, env, 64, 64)
    assert tab.seed(seeds, frontier=fr, query=[0, 1]) == 2
    table.seed(seeds, hashes, query=[0, 1])
    # 15 new keys under the parent of query 0, 5 under query 1's: region 0 is full to the last slot
    host = distinct_list(rng, 15)
    other = distinct_list(rng, 5)
    both = {k: np.concatenate([host[k], other[k]]) for k in ("count", "action", "cost", "hash")}
    both["stride"], both["state"] = 40, np.concatenate([host["state"], other["state"]], axis=1)
    relax_both(m, env, tab, table, both, np.array([0, 1], np.int32), np.zeros(2), fr)
    got = assert_multi_table_equal(tab, table, "just fits")
    assert got["n_nodes"] == 22 and (got["query"] == 0).sum() == 16
    assert np.array_equal(tab.find(got["hash"], got["query"]), np.arange(22, dtype=np.int32))
    assert_spare_untouched(fr)
    # one more key for query 0
    L = upload_lists(m, env, distinct_list(rng, 1))
    pid, pg = upload(env, m, np.zeros(1, np.int32)), upload(env, m, np.zeros(1))
    tab.relax(L, pid, pg, frontier=fr)
    n_nodes, status = tab.stats()
    assert status & m.table.PROBE_FULL and status & m.table.NODES_FULL and n_nodes <= 256
    assert_spare_untouched(fr)
    for call in (lambda: tab.relax(L, pid, pg, frontier=fr), lambda: tab.find([1], 0), lambda: tab.seed(seeds, frontier=fr, query=[0, 1]),
                 lambda: env.alloc_open(tab)):
        with pytest.raises(m._abi.MplxError) as err:
            call()
        assert err.value.code == m._abi.ERR_STATE
    assert tab.stats()[1] == status  # sticky
    tab.clear()
    assert tab.stats() == (0, 0) and tab.seed(seeds, frontier=fr, query=[1, 0]) == 2
    for b in (L, pid, pg, fr):
        b.free()
    tab.free()
    env.close()


def test_one_query_gives_the_bytes_of_the_plain_calls(engine):
    """mplx_table_create_multi(.., 1, ..) with seed_multi (all zeros) and select_multi against the plain calls on the same
    inputs: table, open set, every frontier row and every result."""
    m = engine
    states, goal, in_goal, ignored, push1, push2 = OM.hand_scenario()
    rng = np.random.default_rng(9)
    out = {}
    for form in ("plain", "multi"):
        env = rest_env(m)
        env.set_goal(goal, tol_pos=OM.HAND_TOL)
        if form == "plain":
            tab = env.alloc_table(OM.HAND_N + 600)
        else:
            t = C.c_void_p()
            assert m._abi.lib().mplx_table_create_multi(env._ctx, OM.HAND_N + 600, 1, 0, C.byref(t)) == m._abi.OK
            tab = m.NodeTable.__new__(m.NodeTable)
            tab._env, tab._tab, tab.capacity, tab.n_queries, tab.n_fields = env, t, OM.HAND_N + 600, 1, env.n_fields
            assert tab.query_ptr() is None
        opn = env.alloc_open(tab)
        imp, sel = m.TableFrontier(env, OM.HAND_N), patterned_frontier(m, env, 700, 16)
        cnt = tab.seed(states, frontier=imp, query=None if form == "plain" else np.zeros(OM.HAND_N, np.int32))
        host = OM.hand_frontier(states, push1, with_tail=True)  # (the goal region is dear: the selects are SELECTED)
        fr1 = upload_frontier(m, env, host, len(host["id"]))
        opn.push(fr1, n_max=len(push1["id"]), eps=1.0)
        rows = []
        for delta, cap in ((0.0, 700), (2.5, 700), (40.0, 700)):
            r = opn.select(delta, sel) if form == "plain" else opn.select_many(delta, sel)[0]
            rows.append((r, sel.download()))
        lists = distinct_list(np.random.default_rng(9), 30)
        L = upload_lists(m, env, lists)
        pid, pg = upload(env, m, np.array([3], np.int32)), upload(env, m, np.array([0.5]))
        c2 = tab.relax(L, pid, pg, frontier=imp)
        opn.push(imp, n_max=40, eps=1.0)
        r = opn.select(math.inf, sel) if form == "plain" else opn.select_many(math.inf, sel)[0]
        rows.append((r, sel.download()))
        assert_spare_untouched(sel)
        ids = tab.find(lists["hash"][:30]) if form == "plain" else tab.find(lists["hash"][:30], 0)
        out[form] = (cnt, c2, tab.download(), opn.download(), rows, ids)
        for b in (imp, sel, L, pid, pg, fr1):
            b.free()
        opn.free()
        tab.free()
        env.close()
    (c1, c2, t1, o1, rows1, ids1), (d1, d2, t2, o2, rows2, ids2) = out["plain"], out["multi"]
    assert (c1, c2) == (d1, d2) == (OM.HAND_N, 30) and np.array_equal(ids1, ids2) and ids1.min() >= OM.HAND_N
    for k in t1:
        assert np.asarray(t1[k]).tobytes() == np.asarray(t2[k]).tobytes(), k
    seen = (o1["flags"] & OM.SEEN) > 0
    assert o1["flags"].tobytes() == o2["flags"].tobytes() and o1["f"][seen].tobytes() == o2["f"][seen].tobytes()
    for (r1, f1), (r2, f2) in zip(rows1, rows2):
        assert_result_equal(r2, r1)
        assert_frontier_equal(f2, f1)
    assert rows1[0][0]["status"] == OM.SELECTED and rows1[-1][0]["count"] > 100


def test_argument_errors_and_state(engine):
    m = engine
    L_ = m._abi.lib()
    OK, ARG, STATE = m._abi.OK, m._abi.ERR_ARG, m._abi.ERR_STATE
    env = rest_env(m)
    env._flush()  # (the raw calls below do not go through the wrappers that send the parameters on)
    t = C.c_void_p()
    create = lambda cap, Q, log2, out=t: L_.mplx_table_create_multi(env._ctx, cap, Q, log2, C.byref(out) if out is not None else None)
    for cap, Q, log2 in ((64, 0, 0), (64, -1, 0), (64, 65537, 0), (0, 2, 0), (1 << 31, 2, 0), (64, 2, -1), (64, 2, 32),
                         (64, 2, 31), (64, 65536, 16), (64, 4, 30)):  # the last three: Q * 2^log2 + Q >= 2^32 - 1
        assert create(cap, Q, log2) == ARG, (cap, Q, log2)
    assert L_.mplx_table_create_multi(env._ctx, 64, 2, 0, None) == ARG and L_.mplx_table_create_multi(None, 64, 2, 0, C.byref(t)) == ARG
    tab = env.alloc_table(64, n_queries=3)
    fr = m.TableFrontier(env, 8)
    st = np.zeros((F2, 2))
    st[0] = [0.1, 0.2]
    f = fr.c_struct()
    seed = lambda q, n=2: L_.mplx_table_seed_multi(tab._tab, st.ctypes.data, n, 2, None, q.ctypes.data if q is not None else None, C.byref(f), None)
    for q in ([0, 3], [-1, 0], [0, 1 << 20]):
        assert seed(np.array(q, np.int32)) == ARG, q
    assert seed(None) == ARG and L_.mplx_table_seed_multi(None, st.ctypes.data, 2, 2, None, None, C.byref(f), None) == ARG
    assert tab.stats() == (0, 0)
    # the plain calls on a table with several queries
    ids, h = np.zeros(2, np.int32), np.array([1, 2], np.uint64)
    d_h, d_id = upload(env, m, h), m.DeviceArray(env, 8)
    assert L_.mplx_table_seed(tab._tab, st.ctypes.data, 2, 2, None, C.byref(f), None) == STATE
    assert L_.mplx_table_find(tab._tab, h.ctypes.data, 2, ids.ctypes.data) == STATE
    assert L_.mplx_table_find_device(tab._tab, d_h.ptr, 2, d_id.ptr) == STATE
    assert seed(np.array([2, 0], np.int32)) == OK and tab.stats() == (2, 0)
    q = np.array([0, 3], np.int32)
    assert L_.mplx_table_find_multi(tab._tab, h.ctypes.data, q.ctypes.data, 2, ids.ctypes.data) == ARG
    assert L_.mplx_table_find_multi(tab._tab, h.ctypes.data, None, 2, ids.ctypes.data) == ARG
    assert L_.mplx_table_find_multi_device(tab._tab, d_h.ptr, None, 2, d_id.ptr) == ARG
    p, nq = C.c_void_p(), C.c_int32()
    assert L_.mplx_table_query_of(tab._tab, None, None) == ARG and L_.mplx_table_query_of(None, C.byref(p), C.byref(nq)) == ARG
    assert L_.mplx_table_query_of(tab._tab, C.byref(p), C.byref(nq)) == OK and nq.value == 3 and p.value
    # the open set: push before set_goals, n != Q, the plain select
    opn = env.alloc_open(tab)
    env.set_goal(np.zeros(F2))  # the context's goal does not stand in for the queries' goals
    fr.count.upload(np.array([2], np.int64))
    assert L_.mplx_open_push_device(opn._open, C.byref(f), 2, 1.0, 0) == STATE
    goals = np.zeros((3, F2))
    for n in (2, 4, 0):
        specs = (m._abi.GoalSpec * 4)()
        for k in range(4):
            specs[k].goal, specs[k].control = goals[k % 3].ctypes.data, m.ACC
        assert L_.mplx_open_set_goals(opn._open, specs, n) == ARG, n
    assert L_.mplx_open_set_goals(opn._open, None, 3) == ARG and L_.mplx_open_set_goals(None, specs, 3) == ARG
    specs[1].goal = None
    assert L_.mplx_open_set_goals(opn._open, specs, 3) == ARG
    assert L_.mplx_open_push_device(opn._open, C.byref(f), 2, 1.0, 0) == STATE  # still no goals
    opn.set_goals(goals)
    assert L_.mplx_open_push_device(opn._open, C.byref(f), 2, 1.0, 0) == OK
    assert L_.mplx_open_push_device(opn._open, C.byref(f), 2, 1.0, 1) == STATE  # no map
    res = (m._abi.OpenResult * 3)()
    assert L_.mplx_open_select_device(opn._open, 0.0, C.byref(f), None, res) == STATE
    assert L_.mplx_open_select_multi_device(None, 0.0, C.byref(f), None, res) == ARG
    assert L_.mplx_open_select_multi_device(opn._open, 0.0, None, None, res) == ARG
    for delta in (float("nan"), -0.5):
        assert L_.mplx_open_select_multi_device(opn._open, delta, C.byref(f), None, res) == ARG
    assert L_.mplx_open_select_multi_device(opn._open, 0.0, C.byref(f), None, res) == OK
    # both seeds lie inside their goal regions; query 1 has no node
    assert [r.status for r in res] == [OM.FOUND, OM.EMPTY, OM.FOUND] and sum(r.count for r in res) == 0
    for b in (fr, d_h, d_id):
        b.free()
    opn.free()
    tab.free()
    env.close()
