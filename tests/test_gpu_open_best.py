"""GPU: the k best open nodes per query (include/mplx_best.h) against tests/open_best_model.py.  Every comparison with the
model is bit for bit: the result fields, every frontier row and its order, the spare entries, f and flags of every node
after every call.  Keys are planted as the hand scenario of tests/test_gpu_open.py plants them: states at rest on a
lattice, seeded, then pushed with eps = 0 so f = g."""
import ctypes as C
import math

import numpy as np
import pytest

import multi_model as MM
import open_best_model as BM
import open_model as OM
from helpers import engine_env, oracle_env
from table_model import TableModel, oracle_provider
from test_gpu_multi import assert_query_is_single
from test_gpu_open import (assert_open_equal, assert_result_equal, assert_spare_untouched, corridor_env, patterned_frontier,
                           rest_env, small_world_goal, upload_frontier, _goals)
from test_gpu_table import assert_frontier_equal, assert_table_equal, bits
from test_open import hand_model
from test_open_best import CORRIDOR_BEST, corridor_best

pytestmark = pytest.mark.gpu
INF = math.inf
_hashes = {}


def rest_hashes(O, n):
    if n not in _hashes:
        s = BM.rest_states(n)
        _hashes[n] = [O.lattice_hash(2, O.ACC, s[:, i]) for i in range(n)]
    return _hashes[n]


def far_goal():
    g = np.zeros(10)
    g[:2] = 1000.0
    return g


def select_best_both(opn, model, k, delta, fr, what=""):
    got = opn.select(delta, fr, best=k)
    want, want_fr = model.select_best(k, delta, fr.capacity)
    assert_result_equal(got, want, what)
    assert_frontier_equal(fr.download(), want_fr, what)
    assert_spare_untouched(fr, what)
    assert_open_equal(opn, model, what)
    return got, want_fr


def select_best_many_both(opn, model, k, delta, fr, what=""):
    got = opn.select_many(delta, fr, best=k)
    want, want_fr = model.select_best_many(k, delta, fr.capacity)
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert_result_equal(g, w, "%s: query %d" % (what, q))
    assert_frontier_equal(fr.download(), want_fr, what)
    assert sum(g["count"] for g in got) == want_fr["count"]
    assert_spare_untouched(fr, what)
    assert_open_equal(opn, model, what)
    return got, want_fr


def planted_single(m, O, n):
    """n nodes at rest in a table of one query, nothing pushed: (env, table, open set, model, states)."""
    states = BM.rest_states(n)
    env = rest_env(m)
    env.set_goal(far_goal(), tol_pos=OM.HAND_TOL)
    tab = env.alloc_table(n + 64)
    seeds = m.TableFrontier(env, n)
    assert tab.seed(states, frontier=seeds) == n
    seeds.free()
    table = TableModel(10)
    table.seed(states, rest_hashes(O, n))
    assert table.n_nodes == n
    model = BM.OpenBestModel(table, 2, far_goal(), O.lattice_hash(2, O.ACC, far_goal()), OM.HAND_W, OM.HAND_VMAX, tol_pos=OM.HAND_TOL)
    return env, tab, env.alloc_open(tab), model, states


def test_hand_scenario(engine, oracle_lib):
    """5 000 nodes, one full tile and a partial one, keys from 8 values (eps = 0), so ties are everywhere: k below, at and
    above the capacity, the capacity cut after the k cut, a k that cuts nothing; then push 2 and k = 32 until FOUND."""
    m = engine
    table, model, states, goal, in_goal, ignored, push1, push2 = hand_model(oracle_lib)
    model.__class__ = BM.OpenBestModel
    env = rest_env(m)
    env.set_goal(goal, tol_pos=OM.HAND_TOL)
    tab = env.alloc_table(OM.HAND_N + 100)
    seeds = m.TableFrontier(env, OM.HAND_N)
    assert tab.seed(states, frontier=seeds) == OM.HAND_N
    opn = env.alloc_open(tab)
    host = OM.hand_frontier(states, push1, with_tail=True)
    fr1 = upload_frontier(m, env, host, len(host["id"]))
    opn.push(fr1, n_max=len(push1["id"]), eps=0.0)
    model.push(host, len(push1["id"]), 0.0)
    assert_open_equal(opn, model, "push 1")
    frs = {cap: patterned_frontier(m, env, cap, 64) for cap in (16, 5000)}
    counts = []
    for k, delta, cap in [(1, 0.0, 16), (7, 0.0, 5000), (16, 2.5, 16), (100, INF, 16), (100, INF, 5000), (5000, INF, 5000)]:
        got, _ = select_best_both(opn, model, k, delta, frs[cap], "select_best(%d, %r, %d)" % (k, delta, cap))
        assert got["status"] == OM.SELECTED
        counts.append(got["count"])
    assert counts[:5] == [1, 7, 16, 16, 100] and counts[5] > 1000
    host = OM.hand_frontier(states, push2, with_tail=True)
    fr2 = upload_frontier(m, env, host, len(push2["id"]))
    opn.push(fr2, n_max=10 ** 9, eps=0.0)
    model.push(host, 10 ** 9, 0.0, capacity=len(push2["id"]))
    assert_open_equal(opn, model, "push 2")
    for n in range(400):
        got, _ = select_best_both(opn, model, 32, 2.5, frs[5000], "select %d after push 2" % n)
        if got["status"] != OM.SELECTED:
            break
        assert 1 <= got["count"] <= 32
    assert got["status"] == OM.FOUND and n > 20 and got["count"] == 0
    for b in [seeds, fr1, fr2] + list(frs.values()):
        b.free()
    opn.free()
    tab.free()
    env.close()


@pytest.mark.parametrize("pattern", sorted(BM.key_patterns()))
def test_key_patterns(engine, oracle_lib, pattern):
    """8 229 nodes, two tiles plus 37: per key pattern every k of PATTERN_KS on the freshly planted keys, then the same
    call again on what is left."""
    m = engine
    keys, delta = BM.key_patterns()[pattern]
    n = BM.PATTERN_N
    env, tab, opn, model, states = planted_single(m, oracle_lib, n)
    host = BM.planted(states, keys)
    rows = upload_frontier(m, env, host, n)
    fr = patterned_frontier(m, env, n, 64)
    model.push(host, n, 0.0)
    f0, fl0 = dict(model.f), dict(model.flags)
    for k in BM.PATTERN_KS:
        opn.push(rows, n_max=n, eps=0.0)  # every node open again under its key
        model.f, model.flags = dict(f0), dict(fl0)
        what = "%s, k = %d" % (pattern, k)
        got, sel = select_best_both(opn, model, k, delta, fr, what)
        assert got["status"] == OM.SELECTED and got["count"] == k
        if k < n:  # the k smallest keys: nothing left open is below anything taken
            left = min(model.f[i] for i, fl in model.flags.items() if fl & OM.IS_OPEN)
            assert max(keys[sel["id"]]) <= left
        select_best_both(opn, model, k, delta, fr, what + ", again")
    for b in (rows, fr):
        b.free()
    opn.free()
    tab.free()
    env.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_tables(engine, oracle_lib, n):
    m = engine
    rng = np.random.default_rng(n)
    keys = rng.choice(np.arange(6) * 0.25, n)
    env, tab, opn, model, states = planted_single(m, oracle_lib, n)
    host = BM.planted(states, keys)
    rows = upload_frontier(m, env, host, n)
    fr = patterned_frontier(m, env, n, 16)
    for k in sorted({1, max(n - 1, 1)}):
        opn.push(rows, n_max=n, eps=0.0)
        model.push(host, n, 0.0)
        got, _ = select_best_both(opn, model, k, INF, fr, "n = %d, k = %d" % (n, k))
        assert got["count"] == min(k, n) and got["n_open"] == n - min(k, n)
    for b in (rows, fr):
        b.free()
    opn.free()
    tab.free()
    env.close()


def query_keys(kind, n, k, rng):
    """Keys of one query's n nodes; with delta = 0.5 the candidates are: all (above k), exactly k, k - 3, all (distinct
    keys that differ in their lowest bits), whatever random patterns and powers of two give, one."""
    if kind == 0:
        return np.full(n, 2.5)
    if kind == 1:
        return np.where(rng.permutation(n) < k, 1.0, 7.0)
    if kind == 2:
        return np.where(rng.permutation(n) < k - 3, 1.0, 9.0)
    if kind == 3:
        return (1.0 + np.arange(n) * 2.0 ** -52)[rng.permutation(n)]
    if kind == 4:
        return rng.integers(0, 0x7ff0000000000000, size=n, dtype=np.uint64).view(np.float64)
    if kind == 5:
        expo = np.concatenate([2.0 ** np.arange(-1022, 1024), [0.0, 5e-324, INF]])
        return expo[rng.integers(0, expo.size, size=n)]
    return 10.0 + rng.permutation(n)


@pytest.mark.parametrize("Q", [3, 67])
def test_several_queries(engine, oracle_lib, Q):
    """Interleaved ids (query = id mod Q), another key pattern per query, one query FOUND, one EMPTY, the others with
    candidates below, at and above k; with room for everything and with a capacity below the sum."""
    m, O = engine, oracle_lib
    n = BM.PATTERN_N
    k = 100 if Q == 3 else 41
    rng = np.random.default_rng(Q)
    states = BM.rest_states(n)
    query = (np.arange(n) % Q).astype(np.int32)
    q_found, q_empty = (1, 2) if Q == 3 else (5, 66)
    keys = np.zeros(n)
    for q in range(Q):
        mine = np.nonzero(query == q)[0]
        keys[mine] = query_keys((3, 1, 0)[q] if Q == 3 else q % 7, mine.size, k, rng)
    goals = np.tile(far_goal(), (Q, 1))
    mine = np.nonzero(query == q_found)[0]
    best = mine[np.lexsort((mine, keys[mine].view(np.uint64)))[0]]
    goals[q_found, :2] = states[:2, best]  # its cheapest node lies in its goal region: FOUND
    planted = np.nonzero(query != q_empty)[0]
    env = rest_env(m)
    tab = env.alloc_table(n + 64, n_queries=Q)
    opn = env.alloc_open(tab)
    opn.set_goals(goals, tol_pos=0.01)
    seeds = m.TableFrontier(env, n)
    assert tab.seed(states, frontier=seeds, query=query) == n
    table = MM.MultiTableModel(10, Q)
    table.seed(states, rest_hashes(O, n), query=query)
    model = BM.MultiOpenBestModel(table, 2, goals, [O.lattice_hash(2, O.ACC, g) for g in goals], OM.HAND_W, OM.HAND_VMAX, tol_pos=0.01)
    host = BM.planted(states, keys[planted], planted)
    rows = upload_frontier(m, env, host, planted.size)
    model.push(host, planted.size, 0.0)
    f0, fl0 = dict(model.f), dict(model.flags)
    room, cut = patterned_frontier(m, env, n, 64), patterned_frontier(m, env, (k * (Q - 2)) // 3, 64)
    for delta in (0.5, INF):
        for fr in (room, cut):
            opn.push(rows, n_max=planted.size, eps=0.0)
            model.f, model.flags = dict(f0), dict(fl0)
            what = "Q = %d, delta = %r, capacity %d" % (Q, delta, fr.capacity)
            got, sel = select_best_many_both(opn, model, k, delta, fr, what)
            assert got[q_found]["status"] == OM.FOUND and got[q_found]["goal_id"] == best and got[q_found]["count"] == 0
            assert got[q_empty]["status"] == OM.EMPTY and got[q_empty]["n_open"] == 0
            others = [q for q in range(Q) if q not in (q_found, q_empty)]
            assert all(got[q]["status"] == OM.SELECTED and got[q]["count"] <= k for q in others)
            if fr is room:
                assert all(got[q]["count"] == k for q in others) if (delta == INF or Q == 3) else \
                    {got[q]["count"] for q in others} >= {k, k - 3, 1}
            else:
                assert sel["count"] == cut.capacity and np.all(np.diff(sel["id"]) > 0)
            again, _ = select_best_many_both(opn, model, k, delta, fr, what + ", again")
            assert again[q_found] == got[q_found] and again[q_empty] == got[q_empty]
    for b in (seeds, rows, room, cut):
        b.free()
    opn.free()
    tab.free()
    env.close()


def test_one_query_through_the_multi_form(engine, oracle_lib):
    """The multi form on a table of one query gives the bytes of the plain form."""
    m = engine
    n = 300
    keys = np.random.default_rng(9).choice(np.arange(5) * 0.5, n)
    fronts, opens = [], []
    for multi in (False, True):
        env, tab, opn, model, states = planted_single(m, oracle_lib, n)
        rows = upload_frontier(m, env, BM.planted(states, keys), n)
        opn.push(rows, n_max=n, eps=0.0)
        fr = patterned_frontier(m, env, 64, 16)
        got = opn.select_many(0.5, fr, best=20)[0] if multi else opn.select(0.5, fr, best=20)
        s = fr.state_stride
        fronts.append((got, fr.id.download(np.int32, (s,)), fr.g.download(np.float64, (s,)), fr.state.download(np.float64, (10, s))))
        opens.append(opn.download())
        for b in (rows, fr):
            b.free()
        opn.free()
        tab.free()
        env.close()
    assert fronts[0][0] == fronts[1][0] and fronts[0][0]["count"] == 20
    for a, b in zip(fronts[0][1:], fronts[1][1:]):
        assert a.tobytes() == b.tobytes()
    assert opens[0]["flags"].tobytes() == opens[1]["flags"].tobytes() and opens[0]["f"].tobytes() == opens[1]["f"].tobytes()


def test_equivalence_with_the_plain_select(engine, oracle_lib):
    """Two open sets on twin tables receive the same pushes; a plain select and a best-select with k = the node count
    agree in the frontier's bytes, the flags, f and the results."""
    m = engine
    _, _, states, goal, in_goal, ignored, push1, push2 = hand_model(oracle_lib)
    env = rest_env(m)
    env.set_goal(goal, tol_pos=OM.HAND_TOL)
    tabs, opns, seeds = [], [], m.TableFrontier(env, OM.HAND_N)
    for _ in range(2):
        tabs.append(env.alloc_table(OM.HAND_N + 100))
        assert tabs[-1].seed(states, frontier=seeds) == OM.HAND_N
        opns.append(env.alloc_open(tabs[-1]))
    frs = {cap: [patterned_frontier(m, env, cap, 64) for _ in range(2)] for cap in (0, 16, 5000)}

    def both(delta, cap, what):
        a, b = frs[cap]
        ra, rb = opns[0].select(delta, a), opns[1].select(delta, b, best=OM.HAND_N)
        assert_result_equal(rb, ra, what)
        n = a.state_stride
        for x, y, dt, shape in ((a.id, b.id, np.int32, (n,)), (a.g, b.g, np.float64, (n,)), (a.state, b.state, np.float64, (10, n)),
                                (a.count, b.count, np.int64, (1,))):
            assert x.download(dt, shape).tobytes() == y.download(dt, shape).tobytes(), what
        da, db = opns[0].download(), opns[1].download()
        seen = (da["flags"] & OM.SEEN) > 0  # (f of a node never pushed is unspecified)
        assert da["flags"].tobytes() == db["flags"].tobytes() and da["f"][seen].tobytes() == db["f"][seen].tobytes(), what
        return ra

    host = OM.hand_frontier(states, push1, with_tail=True)
    fr1 = upload_frontier(m, env, host, len(host["id"]))
    for o in opns:
        o.push(fr1, n_max=len(push1["id"]), eps=1.0)
    for delta, cap in OM.HAND_SELECTS:
        both(delta, cap, "select(%r, %d)" % (delta, cap))
    host = OM.hand_frontier(states, push2, with_tail=True)
    fr2 = upload_frontier(m, env, host, len(push2["id"]))
    for o in opns:
        o.push(fr2, n_max=10 ** 9, eps=1.0)
    for n in range(200):
        got = both(2.5, 5000, "select %d after push 2" % n)
        if got["status"] != OM.SELECTED:
            break
    assert got["status"] == OM.FOUND and n > 5
    for o in opns:
        o.clear()
    assert both(0.0, 16, "after clear")["status"] == OM.EMPTY
    for b in [seeds, fr1, fr2] + [f for p in frs.values() for f in p]:
        b.free()
    for o, t in zip(opns, tabs):
        o.free()
        t.free()
    env.close()


def device_search_best(m, env, table, model, start, h0, eps, delta, k, cap, g_max, max_rounds=10 ** 6):
    """device_search of tests/test_gpu_open.py with select_best: every step compared with the model fed with the
    device's own lists."""
    tab = env.alloc_table(1 << 15)
    opn = env.alloc_open(tab)
    sel, imp = patterned_frontier(m, env, cap, 32), m.TableFrontier(env, 1 << 13)
    lists = env.alloc_lists(cap, want_state=True)
    count = tab.seed(start, frontier=imp)
    want_imp, _ = table.seed(start, [h0])
    opn.push(imp, n_max=count, eps=eps, sight=True)
    model.push(want_imp, count, eps, True)
    rounds = 0
    while True:
        what = "round %d" % rounds
        got, want_sel = select_best_both(opn, model, k, delta, sel, what)
        n = got["count"]
        if got["status"] != OM.SELECTED or rounds >= max_rounds:
            break
        env.expand_lists_resident(sel, lists, n_nodes=n)
        cnt = tab.relax(lists, sel.id, sel.g, g_max, frontier=imp, n_nodes=n)
        want_imp, _ = table.relax(lists.download_nodes(0, n), want_sel["id"], want_sel["g"], g_max)
        assert_frontier_equal(imp.download(cnt), want_imp, what + ": relax")
        opn.push(imp, n_max=n * lists.stride, eps=eps, sight=True)
        model.push(want_imp, n * lists.stride, eps, True)
        rounds += 1
    for b in (sel, imp, lists):
        b.free()
    return tab, opn, got, rounds


@pytest.mark.parametrize("case", [(1.0, INF, 1, 8192), (1.0, INF, 16, 8192), (1.0, 5.0, 16, 16), (3.0, INF, 64, 8192)])
@pytest.mark.parametrize("world", [(2, 0x03, 56.0, 32), (3, 0x07, 46.0, 64)])
def test_search_round_by_round(engine, oracle_lib, world, case):
    """2D ACC and 3D JRK to FOUND with the ray trace: the device loop with `best` against the model loop, every round's
    selection, table and open set; the rounds and expansions are the model's on the oracle's successors."""
    m, O = engine, oracle_lib
    dim, control, g_max, edge = world
    eps, delta, k, cap = case
    if world not in _goals:
        _goals[world] = small_world_goal(m, O, dim, control, g_max, edge)
    wl, start, h0, goal = _goals[world]
    env = engine_env(m, wl)
    env.set_goal(goal, tol_pos=wl.res)

    def models():
        table = TableModel(4 * dim + 2)
        return table, BM.OpenBestModel(table, dim, goal, O.lattice_hash(dim, control, goal), env._p.w, env._p.v_max, tol_pos=wl.res,
                                       blocked=OM.ray_blocked(wl.grid, wl.map_dim, wl.origin, wl.res, goal[:dim]))
    t2, m2 = models()
    want = BM.search_best(t2, m2, oracle_provider(O, oracle_env(wl)), start, h0, eps, delta, k, cap, g_max=g_max, sight=True)
    table, model = models()
    tab, opn, got, rounds = device_search_best(m, env, table, model, start, h0, eps, delta, k, cap, g_max)
    print(world, case, rounds, got, want)
    assert got["status"] == OM.FOUND == want["status"] and rounds == want["rounds"] and rounds >= 3
    assert_result_equal(got, want["result"])
    assert_table_equal(tab, table)
    opn.free()
    tab.free()
    env.close()


def test_corridor_end_to_end(engine, monkeypatch):
    """EnvMap.search(best=16, delta=inf) on the corridor of test_planner_2d: the published cost with the model's rounds,
    expansions and nodes, a path the rollout accepts, lists of min(capacity, best * Q) rows, a replan that keeps `best`,
    and search_many with 8 shifted queries, each its own single search."""
    m = engine
    env, start, goal = corridor_env(m)
    rounds, expanded, nodes, goal_f = CORRIDOR_BEST[(1.0, INF, 16)]
    table, _, want = corridor_best(m, 1.0, INF, 16)
    asked, selects = [], []
    alloc, select, select_many = m.EnvMap.alloc_lists, m.search.OpenSet.select, m.search.OpenSet.select_many
    monkeypatch.setattr(m.EnvMap, "alloc_lists", lambda self, n, *a, **kw: (asked.append(n), alloc(self, n, *a, **kw))[1])
    monkeypatch.setattr(m.search.OpenSet, "select", lambda self, *a, **kw: (selects.append(kw.get("best")), select(self, *a, **kw))[1])
    monkeypatch.setattr(m.search.OpenSet, "select_many",
                        lambda self, *a, **kw: (selects.append(kw.get("best")), select_many(self, *a, **kw))[1])
    kw = dict(eps=1.0, delta=INF, sight=False, capacity=1 << 15, best=16)
    res = env.search(start, goal, **kw)
    print(res, res.last_select)
    assert res.found and res.cost == 351.5 and (res.rounds, res.expanded) == (rounds, expanded)
    assert_result_equal(res.last_select, want["result"])
    assert assert_table_equal(res.table, table)["n_nodes"] == nodes
    assert asked == [16] and selects == [16] * (rounds + 1)
    start_state, act = res.path()
    r = env.rollout(start_state, act.reshape(-1, 1))
    assert len(act) == 35 and r["status"][0] == m.SLOT_FINITE and r["steps"][0] == 35 and bits(r["cost"])[0] == bits([351.5])[0]
    del selects[:]
    again = res.replan(advance=5)
    assert again.found and again.cost == 351.5 and selects and set(selects) == {16}
    again.free()
    # 8 queries shifted along free cells: no selection is cut at the capacity, so each equals its own single search
    # (tests/test_multi.py::corridor_queries: 0.5 m up from the start and 0.5 m down from the goal are free cells)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    starts = np.stack([wp(start[:2] + [0.0, 0.5 * j / 7]) for j in range(8)], axis=1)
    goals = np.stack([wp(goal[:2] - [0.0, 0.5 * j / 7]) for j in range(8)])
    del asked[:]
    multi = env.search_many(starts, goals, **kw)
    assert asked == [128] and multi.found[0] and multi.found[7] and multi.cost[0] == 351.5
    for q in range(8):
        single = env.search(starts[:, q], goals[q], **kw)
        assert_query_is_single(multi, q, single, "query %d" % q)
        single.free()
    multi.free()
    capped = env.search(start, goal, max_frontier=4096, **kw)  # an explicit max_frontier decides
    assert asked[-1] == 4096 and capped.cost == 351.5 and capped.rounds == rounds
    capped.free()
    env.close()


def test_argument_errors_and_state(engine, oracle_lib):
    m = engine
    L_ = m._abi.lib()
    ARG, STATE, OK = m._abi.ERR_ARG, m._abi.ERR_STATE, m._abi.OK
    n = 200
    keys = np.random.default_rng(4).choice(np.arange(4) * 1.0, n)
    env, tab, opn, model, states = planted_single(m, oracle_lib, n)
    host = BM.planted(states, keys)
    rows = upload_frontier(m, env, host, n)
    opn.push(rows, n_max=n, eps=0.0)
    model.push(host, n, 0.0)
    fr, none = patterned_frontier(m, env, 32, 16), patterned_frontier(m, env, 0, 16)
    res = m._abi.OpenResult()

    def best(k=4, delta=0.0, f=None, o=opn._open, fn=L_.mplx_open_select_best_device):
        f = fr.c_struct() if f is None else f
        return fn(o, k, delta, C.byref(f), None, C.byref(res))
    for fn in (L_.mplx_open_select_best_device, L_.mplx_open_select_best_multi_device):
        for k in (0, -1, -2 ** 40):
            assert best(k=k, fn=fn) == ARG, k
        for delta in (float("nan"), -0.5, -INF):
            assert best(delta=delta, fn=fn) == ARG, delta
        assert best(o=None, fn=fn) == ARG and fn(opn._open, 4, 0.0, None, None, None) == ARG
        for field, v in (("id", None), ("g", None), ("state", None), ("count", None), ("state_stride", 7), ("capacity", -1)):
            f = fr.c_struct()
            setattr(f, field, v)
            assert best(f=f, fn=fn) == ARG, field
    assert_open_equal(opn, model, "after the errors")  # nothing of the above touched anything
    # a frontier without rows: as the plain select answers it -- SELECTED, nothing taken
    got, _ = select_best_both(opn, model, 4, 0.0, none, "capacity 0")
    assert got["status"] == OM.SELECTED and got["count"] == 0 and got["n_open"] == n
    got, _ = select_best_both(opn, model, 4, 0.0, fr, "the first that works")
    assert got["count"] == 4
    # the single form on a table with Q > 1
    tab3 = env.alloc_table(64, n_queries=3)
    opn3 = env.alloc_open(tab3)
    assert best(o=opn3._open) == STATE
    res3 = (m._abi.OpenResult * 3)()  # (the multi form writes Q results)
    assert L_.mplx_open_select_best_multi_device(opn3._open, 4, 0.0, C.byref(fr.c_struct()), None, res3) == OK
    assert [r.status for r in res3] == [OM.EMPTY] * 3
    # a table with a status bit: 40 new keys into 8 free nodes
    from test_gpu_table import distinct_list, upload, upload_lists
    lists = upload_lists(m, env, distinct_list(np.random.default_rng(3), 40))
    pid, pg = upload(env, m, np.zeros(1, np.int32)), upload(env, m, np.zeros(1))
    small = env.alloc_table(8)
    sopn = env.alloc_open(small)
    big = m.TableFrontier(env, 64)
    small.relax(lists, pid, pg, frontier=big, want_count=False)
    with pytest.raises(m._abi.MplxError) as err:
        sopn.select(0.0, big, best=3)
    assert err.value.code == STATE and small.stats()[1] & m.table.NODES_FULL
    with pytest.raises(m._abi.MplxError) as err:
        sopn.select_many(0.0, big, best=3)
    assert err.value.code == STATE
    small.clear()
    sopn.clear()
    assert sopn.select(0.0, big, best=3)["status"] == OM.EMPTY
    for b in (rows, fr, none, lists, pid, pg, big):
        b.free()
    for o, t in ((sopn, small), (opn3, tab3), (opn, tab)):
        o.free()
        t.free()
    env.close()
