"""GPU: include/mplx_anytime.h -- mplx_open_rekey_device against tests/anytime_model.py bit for bit, the identity of a
re-key at a search's own eps, and SearchResult / MultiSearchResult .bound() / .improve() and search.anytime on small
maps against fresh searches.  Every test here fails without the feature: the symbol and the methods do not exist."""
import ctypes as C
import math

import numpy as np
import pytest

import anytime_model as AM
import field_model as FM
import heur_model as HM
import multi_model as MM
import open_model as OM
import prior_model as PM
from test_gpu_field import map_env, push_world
from test_gpu_open import corridor_env
from test_multi import corridor_queries

pytestmark = pytest.mark.gpu

W, VMAX = 1.0, 2.0
EPS0 = 1.5  # the eps of the pushes that build a table


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def code(m, fn):
    with pytest.raises(m._abi.MplxError) as e:
        fn()
    return e.value.code


class Stub:
    """What the models read of a table: the device table's own arrays."""

    def __init__(self, d, Q):
        self.hash, self.g, self.state, self.query = d["hash"], d["g"], d["state"], d["query"]
        self.n_nodes, self.n_queries, self.n_fields = d["n_nodes"], Q, d["state"].shape[0]


def lattice_states(D, F, K, Q, goals, rng, control):
    """K distinct lattice states at rest (multiples of 0.25 m, in shuffled order), a random query and one of eight g
    values each; row q < Q is the goal's own state of query q (as far as K reaches).  waypoint.h's hash collides for
    some small lattice states: a candidate whose (query, hash) is taken is passed over."""
    s = np.zeros((F, K))
    query = rng.integers(0, Q, K).astype(np.int32)
    taken, n = set(), 0
    for q in range(min(Q, K)):
        s[:, q], query[q] = goals[q], q
        taken.add((q, PM.lattice_hash(D, control, [float(x) for x in goals[q]])))
        n += 1
    for k in rng.permutation(K + Q + 512):
        if n == K:
            break
        col = np.zeros(F)
        col[0], col[1] = 0.25 * (k % 64), 0.25 * (k // 64 if D == 2 else (k // 64) % 16)
        if D == 3:
            col[2] = 0.25 * (k // 1024)
        key = (int(query[n]), PM.lattice_hash(D, control, [float(x) for x in col]))
        if key in taken:
            continue
        taken.add(key)
        s[:, n] = col
        n += 1
    assert n == K
    s[4 * D + 1] = rng.integers(0, 7, K).astype(np.float64)  # t: what priors read
    g = rng.integers(0, 8, K) * 0.5
    return s, query, g


def goals_of(D, F, Q):
    g = np.zeros((Q, F))
    for q in range(Q):
        g[q, 0], g[q, 1] = 20.0 + 0.25 * (q % 8) + 0.125, 1.0 + 0.25 * (q // 8) + 0.125  # (off the lattice of the states)
    return g


def build(m, env, D, Q, K, seed, own_goals=False, tol=0.5):
    """A table of K seeds, for reset() to push.  Returns what a test needs."""
    F = env.n_fields
    goals = goals_of(D, F, Q)
    states, query, g = lattice_states(D, F, K, Q, goals, np.random.default_rng(seed), m.ACC)
    tab = env.alloc_table(max(K, 64) + 64, n_queries=Q)
    opn = env.alloc_open(tab)
    multi = Q > 1 or own_goals
    if multi:
        opn.set_goals(goals, w=W, v_max=VMAX, tol_pos=tol)
    else:
        env.set_goal(goals[0], w=W, v_max=VMAX, tol_pos=tol)
    fr = m.TableFrontier(env, K)
    assert tab.seed(states, g, frontier=fr, query=query if Q > 1 else None) == K
    return dict(tab=tab, opn=opn, fr=fr, goals=goals, multi=multi, Q=Q, K=K, D=D)


def reset(b):
    """The same open set every time: everything pushed open, then the first half of the rows pushed closed."""
    opn = b["opn"]
    opn.clear()
    opn.push(b["fr"], n_max=b["K"], eps=EPS0)
    opn.push(b["fr"], n_max=b["K"] // 2, eps=EPS0, closed=True)


def model_of(b, d, ctl, h_of=None, heur=None):
    D, Q, goals = b["D"], b["Q"], b["goals"]
    stub = Stub(d, Q)
    gh = [PM.lattice_hash(D, ctl, [float(x) for x in goals[q]]) for q in range(Q)]
    if heur == "robust":
        mo = HM.HeurMultiOpenModel(stub, D, goals, gh, W, VMAX, control=ctl, goal_controls=[0] * Q, tol_pos=0.5) if b["multi"] else \
            HM.HeurOpenModel(stub, D, goals[0], gh[0], W, VMAX, control=ctl, goal_control=0, tol_pos=0.5)
    elif b["multi"]:
        mo = MM.MultiOpenModel(stub, D, goals, gh, W, VMAX, tol_pos=0.5)
    else:
        mo = OM.OpenModel(stub, D, goals[0], gh[0], W, VMAX, tol_pos=0.5)
    # h once per node: the same IEEE operations as one call per re-key, only faster
    h = [float(h_of(i, stub.state[:, i]) if h_of else mo.heur_and_tol(i, stub.state[:, i])[0]) for i in range(stub.n_nodes)]
    return stub, mo, h, gh


def check_rekeys(m, b, mo, stub, h, what):
    """Every (eps, write, cut) on the same open set, device against model: f, flags and every field of the bound."""
    opn, Q, K = b["opn"], b["Q"], b["K"]
    h_of = lambda i, s: h[i]
    reset(b)
    d0 = opn.download()
    start = ({i: float(d0["f"][i]) for i in range(K)}, {i: int(d0["flags"][i]) for i in range(K)})
    assert np.all(d0["flags"] & OM.SEEN)
    n_open0 = int(np.sum((d0["flags"] & OM.IS_OPEN) > 0))
    assert n_open0 == K - K // 2  # open and closed nodes both
    # the cut: per query the median L of its open nodes -- an exact tie with that node
    cut = []
    for q in range(Q):
        Ls = sorted(float(stub.g[i]) + h[i] for i in range(K) if (start[1][i] & OM.IS_OPEN) and (Q == 1 or stub.query[i] == q)
                    and h[i] == h[i])
        cut.append(Ls[len(Ls) // 2] if Ls else math.inf)
    pruned_any = 0
    for eps in (0.0, 1.0, 2.5):
        for write in (False, True):
            for c in (None, cut):
                reset(b)
                got = opn.rekey(eps, cut=c, write=write)
                dev = opn.download()
                mo.f, mo.flags = dict(start[0]), dict(start[1])
                want = AM.rekey(mo, eps, write, c, Q, h_of=h_of)
                w = "%s eps %r write %r cut %r" % (what, eps, write, c is not None)
                for q in range(Q):
                    assert got[q]["n_open"] == want[q]["n_open"] and got[q]["n_pruned"] == want[q]["n_pruned"], (w, q, got[q], want[q])
                    assert got[q]["n_rekeyed"] == want[q]["n_rekeyed"], (w, q, got[q], want[q])
                    assert bits([got[q]["lower"]])[0] == bits([want[q]["lower"]])[0], (w, q, got[q], want[q])
                assert np.array_equal(dev["flags"], np.array([mo.flags[i] for i in range(K)], np.uint8)), w
                assert np.array_equal(bits(dev["f"]), bits([mo.f[i] for i in range(K)])), w
                if not write:
                    assert np.array_equal(dev["flags"], d0["flags"]) and np.array_equal(bits(dev["f"]), bits(d0["f"])), w
                elif c is not None:
                    pruned_any += sum(x["n_pruned"] for x in got)
    assert pruned_any > 0, what
    return cut


def free(b):
    for k in ("fr", "opn", "tab"):
        b[k].free()


# ---- 1. model parity
@pytest.mark.parametrize("D,Q", [(2, 1), (2, 3), (2, 67), (3, 1), (3, 3), (3, 67)])
def test_rekey_equals_the_model(engine, D, Q):
    m = engine
    dims, res, cells = push_world(D)
    env = map_env(m, dims, cells, res=res, control=m.ACC, vals=(-0.5, 0.0, 0.5), v_max=VMAX)
    for K in (1, 63, 64, 65, 255, 256, 257, 4097):
        b = build(m, env, D, Q, K, 100 * D + Q + K)
        stub, mo, h, gh = model_of(b, b["tab"].download(), m.ACC)
        if K >= Q:
            goal_nodes = [i for i in range(K) if int(stub.hash[i]) == gh[int(stub.query[i])]]
            assert len(goal_nodes) >= min(Q, K) and all(h[i] == 0.0 for i in goal_nodes)  # the goal's own lattice state
        check_rekeys(m, b, mo, stub, h, "D %d Q %d K %d" % (D, Q, K))
        free(b)
    env.close()


def test_rekey_with_robust_equals_the_model(engine):
    m = engine
    dims, res, cells = push_world(2)
    env = map_env(m, dims, cells, res=res, control=m.ACC, vals=(-0.5, 0.0, 0.5), v_max=VMAX)
    b = build(m, env, 2, 3, 257, 5)
    b["opn"].set_heur("robust")
    stub, mo, h, _ = model_of(b, b["tab"].download(), m.ACC, heur="robust")
    stub_d, mo_d, h_d, _ = model_of(b, b["tab"].download(), m.ACC)
    check_rekeys(m, b, mo, stub, h, "robust")
    assert all(a >= c for a, c in zip(h, h_d))
    free(b)
    env.close()


def test_rekey_with_robust_differs_from_the_default_on_moving_states(engine):
    """ROBUST on states with a velocity: keys above the default's, and the re-key follows the push bit for bit."""
    m = engine
    dims, res, cells = push_world(2)
    env = map_env(m, dims, cells, res=res, control=m.ACC, vals=(-0.5, 0.0, 0.5), v_max=VMAX)
    F, K = env.n_fields, 200
    rng = np.random.default_rng(3)
    s = np.zeros((F, K))
    s[0], s[1] = 0.25 * np.arange(K), 0.25 * rng.integers(0, 30, K)
    s[2:4] = rng.integers(-4, 5, (2, K)) / 4.0
    goal = goals_of(2, F, 1)[0]
    tab = env.alloc_table(512)
    opn = env.alloc_open(tab)
    env.set_goal(goal, w=W, v_max=VMAX, tol_pos=0.5)
    opn.set_heur("robust")
    fr = m.TableFrontier(env, K)
    n = tab.seed(s, rng.integers(0, 8, K) * 0.5, frontier=fr)
    opn.push(fr, n_max=K, eps=2.0)
    d0 = opn.download()
    b0 = opn.rekey(2.0)
    d1 = opn.download()
    assert np.array_equal(bits(d0["f"]), bits(d1["f"])) and np.array_equal(d0["flags"], d1["flags"]) and b0[0]["n_rekeyed"] == n
    opn.set_heur(None)
    opn.rekey(2.0)
    d2 = opn.download()
    assert np.all(d2["f"] <= d1["f"]) and int(np.sum(d2["f"] < d1["f"])) > n // 2
    for x in (fr, opn, tab):
        x.free()
    env.close()


def test_rekey_with_a_field_equals_the_model(engine):
    m = engine
    D, Q = 2, 1
    dims, res, cells = push_world(D)
    env = map_env(m, dims, cells, res=res, control=m.ACC, vals=(-0.5, 0.0, 0.5), v_max=VMAX)
    F = env.n_fields
    K = 257
    goal = np.zeros((1, F))
    goal[0, :2] = [(dims[0] - 3 + 0.5) * res, 1.5 * res]
    rng = np.random.default_rng(9)
    s = np.zeros((F, K))
    k = rng.permutation(dims[0] * dims[1] * 4)[:K]
    s[0], s[1] = 0.25 * (k % (2 * dims[0])) + 0.01, 0.25 * (k // (2 * dims[0])) + 0.01  # on and off the map's cells, behind the wall
    s[:, 0] = goal[0]
    g = rng.integers(0, 8, K) * 0.5
    tab = env.alloc_table(512)
    opn = env.alloc_open(tab)
    env.set_goal(goal[0], w=W, v_max=VMAX, tol_pos=0.5)
    fld = env.alloc_field().build(goal, 0.5)
    opn.set_field(fld)
    fr = m.TableFrontier(env, K)
    assert tab.seed(s, g, frontier=fr) == K
    b = dict(tab=tab, opn=opn, fr=fr, goals=goal, multi=False, Q=1, K=K, D=D)
    d = tab.download()
    gh = PM.lattice_hash(D, m.ACC, [float(x) for x in goal[0]])
    dist = fld.dist()
    h_of = lambda i, col: float(FM.heuristic(col[:D], goal[0], W, VMAX, dist[0], dims, [0.0] * D, res, int(d["hash"][i]) == gh)[0])
    stub, mo, h, _ = model_of(b, d, m.ACC, h_of=h_of)
    plain = [mo.heur_and_tol(i, stub.state[:, i])[0] for i in range(K)]
    assert sum(a > c for a, c in zip(h, plain)) >= 10 and h[0] == 0.0  # the field's detour counts; the goal's own state
    check_rekeys(m, b, mo, stub, h, "field")
    free(b)
    fld.free()
    env.close()


def test_rekey_with_priors_equals_the_model(engine):
    m = engine
    env, start, goal = wall_env(m)
    r1 = env.search(start, goal, capacity=1 << 14, sight=False)
    assert r1.found
    prior = r1.as_prior()
    r1.free()
    D, K = 2, 257
    b = build(m, env, D, 1, K, 77, own_goals=True)
    info = b["opn"].set_prior_list([prior])
    assert info["n_steps"][0] > 3
    pr = b["opn"].priors()
    d = b["tab"].download()
    stub = Stub(d, 1)
    p = {"n_steps": int(pr["n_steps"][0]), "pos": pr["pos"][0], "togo": pr["togo"][0], "goal_row": pr["goal_row"][0],
         "goal_hash": int(pr["goal_hash"][0])}
    mo = PM.PriorMultiOpenModel(stub, D, b["goals"], [0], W, VMAX, float(env._p.dt), [p], tol_pos=0.5)
    h = [float(mo.heur_and_tol(i, stub.state[:, i])[0]) for i in range(K)]
    plain = MM.MultiOpenModel(stub, D, [p["goal_row"]], [p["goal_hash"]], W, VMAX, tol_pos=0.5)
    assert sum(h[i] != plain.heur_and_tol(i, stub.state[:, i])[0] for i in range(K)) > K // 4  # the prior leads, by the time row
    check_rekeys(m, b, mo, stub, h, "priors")
    free(b)
    env.close()


# ---- the small maps of 2., 4., 6., 7.
def wall_env(m, D=2, w=None):
    """48 x 32 cells (16^3 in 3-D) of 0.25 m; ACC, u in {-0.5, 0, 0.5}, dt 1, v_max 1: a lattice of 0.25 m."""
    dims = [48, 32] if D == 2 else [16, 16, 16]
    env = map_env(m, dims, AM.wall_cells(dims), res=0.25, control=m.ACC, vals=(-0.5, 0.0, 0.5), v_max=1.0)
    if w is not None:
        env.set_w(w)
    p0, p1 = AM.wall_query(dims)
    start, goal = m.Waypoint(D, m.ACC, pos=p0).to_row(), m.Waypoint(D, m.ACC, pos=p1).to_row()
    return env, start, goal


def assert_identity(res, eps, what):
    d0 = res.open.download()
    n = d0["n_nodes"]
    got = res.open.rekey(eps)
    d1 = res.open.download()
    seen = (d0["flags"] & OM.SEEN) > 0
    assert n > 20 and np.array_equal(d0["flags"], d1["flags"]), what
    assert np.array_equal(bits(d0["f"][seen]), bits(d1["f"][seen])), what
    v = res.open.view()  # every byte: the keys of nodes that were never pushed too
    raw0 = res.table._read(v.f, np.uint64, n)
    res.open.rekey(eps)
    assert np.array_equal(raw0, res.table._read(v.f, np.uint64, n)), what
    assert sum(x["n_rekeyed"] for x in got) == int(seen.sum()) and sum(x["n_pruned"] for x in got) == 0, what
    assert sum(x["n_open"] for x in got) == int(np.sum((d0["flags"] & OM.IS_OPEN) > 0)), what


# ---- 2. identity
IDENTITY = ["wall", "3d", "max_rounds", "Q3", "field", "robust", "priors", "sight", "timed"]


@pytest.mark.parametrize("name", IDENTITY)
def test_rekey_at_the_search_eps_is_the_identity(engine, name):
    m = engine
    eps = 2.0
    env, start, goal = wall_env(m, 3 if name == "3d" else 2)
    kw = dict(eps=eps, capacity=1 << 15, sight=(name == "sight"))
    avoid = None
    if name == "max_rounds":
        res = env.search(start, goal, max_rounds=3, **kw)
        assert res.status == m.search.MAX_ROUNDS
    elif name == "Q3":
        starts = np.stack([start] * 3, axis=1)
        starts[1] += [0.5, 0.25, 0.0]
        goals = np.stack([goal] * 3)
        goals[:, 1] -= [0.0, 0.5, 1.0]
        res = env.search_many(starts, goals, **kw)
    elif name == "priors":
        r1 = env.search(start, goal, **kw)
        prior = r1.as_prior()
        r1.free()
        res = env.search(start, goal, prior=prior, **kw)
    elif name == "timed":
        other = env.search(goal, start, **kw)  # a robot coming the other way
        p = other.path()
        avoid = env.alloc_reservations((p[0].reshape(-1, 1), p[1].reshape(-1, 1)), 0.5, n_steps=200, radius=0.3)
        other.free()
        res = env.search(start, goal, avoid=avoid, radius=0.3, wait=True, **kw)
    else:
        res = env.search(start, goal, field=True if name == "field" else None, heur="robust" if name == "robust" else None, **kw)
    if name != "max_rounds":
        assert np.all(res.found)
    print(name, res)
    assert_identity(res, eps, name)
    res.free()
    if avoid is not None:
        avoid.free()
    env.close()


# ---- 3. write = 0, errors, state
def test_write_zero_errors_and_a_table_with_a_status_bit(engine):
    m = engine
    A = m._abi
    env, start, goal = wall_env(m)
    res = env.search(start, goal, eps=2.0, max_rounds=3, capacity=256, sight=False)
    assert res.status == m.search.MAX_ROUNDS
    opn, tab = res.open, res.table
    n = tab.stats()[0]
    v = opn.view()
    raw = lambda: (tab._read(v.f, np.uint64, opn.capacity).copy(), tab._read(v.flags, np.uint8, opn.capacity).copy())
    f0, fl0 = raw()
    b = opn.rekey(1.0, write=False, cut=[0.0])
    f1, fl1 = raw()
    assert np.array_equal(f0, f1) and np.array_equal(fl0, fl1)  # no byte, whatever the cut
    assert b[0]["n_open"] == int(np.sum((fl0[:n] & OM.IS_OPEN) > 0)) > 0 and b[0]["n_pruned"] == 0 and b[0]["n_rekeyed"] == 0
    assert b[0]["lower"] == res.bound()["lower"] + res.bound()["slack"]
    rk = lambda o=opn._open, eps=1.0, cut=None, hb=None: A.check(env._ctx, A.lib().mplx_open_rekey_device(o, eps, 1, cut, None, hb))
    assert A.lib().mplx_open_rekey_device(None, 1.0, 1, None, None, None) == A.ERR_ARG
    for bad in (-1.0, math.nan, math.inf):
        assert code(m, lambda: rk(eps=bad)) == A.ERR_ARG
    for bad in (math.nan, -0.5):
        c = (C.c_double * 1)(bad)
        assert code(m, lambda: rk(cut=C.cast(c, C.c_void_p))) == A.ERR_ARG
    f2, fl2 = raw()
    assert np.array_equal(f0, f2) and np.array_equal(fl0, fl2)  # a call that fails changes nothing
    assert opn.rekey(1.0, cut=math.inf)[0]["n_pruned"] == 0  # +inf prunes nothing
    # an empty table: a no-op with lower = +inf; without a goal: ERR_STATE
    env2 = m.EnvMap(2)
    t2 = env2.alloc_table(64)
    o2 = env2.alloc_open(t2)
    assert code(m, lambda: o2.rekey(1.0)) == A.ERR_STATE
    env2.set_control(m.ACC)
    env2.set_goal(goal)
    assert o2.rekey(1.0) == [{"lower": math.inf, "n_open": 0, "n_pruned": 0, "n_rekeyed": 0}]
    o2.free()
    t2.free()
    env2.close()
    # a status bit: rounds on a table of 256 nodes until it is full
    lists = env.alloc_lists(256, want_state=True)
    sel, imp = m.TableFrontier(env, 256), m.TableFrontier(env, 256)
    for _ in range(40):
        got = opn.select(math.inf, sel)
        if got["status"] != m.search.SELECTED:
            break
        env.expand_lists_resident(sel, lists, n_nodes=got["count"])
        tab.relax(lists, sel.id, sel.g, frontier=imp, n_nodes=got["count"], want_count=False)
        opn.push(imp, n_max=got["count"] * lists.stride, eps=2.0)
        if tab.stats()[1]:
            break
    assert tab.stats()[1] & m.table.NODES_FULL
    f3, fl3 = raw()
    assert code(m, lambda: opn.rekey(1.0)) == A.ERR_STATE and code(m, lambda: opn.rekey(1.0, write=False)) == A.ERR_STATE
    with pytest.raises(m._abi.MplxError):
        res.bound()
    with pytest.raises((m._abi.MplxError, RuntimeError)):
        res.improve(1.0)
    assert res.table is not None  # the result still owns its table
    f4, fl4 = raw()
    assert np.array_equal(f3, f4) and np.array_equal(fl3, fl4)
    for x in (lists, sel, imp):
        x.free()
    res.free()
    env.close()


# ---- 4. the schedule on the wall map, zero tolerances, w = 1
def test_schedule_on_the_wall_map(engine):
    m = engine
    env, start, goal = wall_env(m, w=1.0)
    kw = dict(delta=0.0, capacity=1 << 16, tol_pos=0.0, sight=False)
    fresh = env.search(start, goal, eps=1.0, **kw)
    assert fresh.found
    res = env.search(start, goal, eps=4.0, **kw)
    b = res.bound()
    stages = [dict(eps=4.0, cost=[res.cost], lower=[b["lower"]], ratio=[b["ratio"]], expanded=[res.expanded], rounds=[res.rounds])]
    assert b["certified"] and b["slack"] == 0.0
    res, more = m.search.anytime(res, [2.0, 1.0])
    stages += more
    print("fresh", fresh.cost, fresh.rounds, fresh.expanded)
    for s in stages:
        print(s)
    costs = [s["cost"][0] for s in stages]
    assert all(b <= a for a, b in zip(costs, costs[1:])) and costs[0] < math.inf
    for s in stages:
        assert s["cost"][0] <= s["eps"] * s["lower"][0] * (1 + 1e-12), s
    assert bits([res.cost])[0] == bits([fresh.cost])[0]  # (a stage that proves its cost optimal ends the schedule)
    assert res.bound()["ratio"] <= 1 + 1e-12
    assert res.expanded == sum(s["expanded"][0] for s in stages) and res.rounds == sum(s["rounds"][0] for s in stages)
    s0, act = res.path()
    out = env.rollout(s0, act.reshape(-1, 1))
    assert out["status"][0] == m.SLOT_FINITE and bits(out["cost"])[0] == bits([res.cost])[0]
    with pytest.raises(ValueError):
        m.search.anytime(res, [1.0, 2.0])
    fresh.free()
    res.free()
    env.close()


# ---- 5. the same on the corridor of test_planner_2d, with its 0.5 m tolerance
def test_schedule_on_the_corridor(engine):
    m = engine
    env, start, goal = corridor_env(m)
    kw = dict(capacity=1 << 16)
    fresh = env.search(start, goal, eps=1.0, **kw)
    assert fresh.found and fresh.cost == 351.5
    res = env.search(start, goal, eps=4.0, **kw)
    b = res.bound()
    slack = b["slack"]
    assert slack == 10.0 * 0.5 / 1.0 and b["certified"]
    seen = [(4.0, res.cost, b["lower"])]
    res, stages = env.anytime(res, [2.0, 1.0])
    seen += [(s["eps"], s["cost"][0], s["lower"][0]) for s in stages]
    print("fresh", fresh.cost, fresh.expanded, seen, [s["expanded"] for s in stages])
    costs = [c for _, c, _ in seen]
    assert all(b <= a for a, b in zip(costs, costs[1:]))
    for eps, cost, lower in seen:
        assert lower - slack <= fresh.cost, (eps, cost, lower)
    assert abs(res.cost - fresh.cost) <= slack
    fresh.free()
    res.free()
    env.close()


# ---- 6. batches
def test_improve_of_a_batch_is_every_query_improved_alone(engine):
    from test_gpu_multi import assert_query_is_single
    m = engine
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    kw = dict(eps=3.0, delta=0.0, capacity=1 << 16)
    multi = env.search_many(starts, goals, **kw).improve(1.0)
    assert multi.found == [True] * 3
    for q in range(3):
        single = env.search(starts[:, q], goals[q], **kw).improve(1.0)
        assert_query_is_single(multi, q, single, "query %d" % q)
        assert multi.rekey_info[q]["n_pruned"] == single.rekey_info[0]["n_pruned"]
        bm, bs = multi.bound()[q], single.bound()
        assert bits([bm["lower"]])[0] == bits([bs["lower"]])[0] and bm["certified"] and bs["certified"]
        single.free()
    multi.free()
    env.close()


# ---- 7. improve, then replan
def test_improve_then_replan(engine):
    """(At eps = 1 the equality with a fresh search is what tests/test_gpu_replan.py pins for replan itself; above it
    both costs are only within eps of the optimum, and differ: 353.0 against 352.0 at eps = 1.5.)"""
    from test_replan import DELTA, EPS, world
    m = engine
    w = world(m)
    env, start, goal = corridor_env(m)
    kw = dict(delta=DELTA, capacity=1 << 15, sight=False)
    r0 = env.search(start, goal, eps=3.0, **kw)
    r1 = r0.improve(EPS)
    assert r0.table is None and r1.found and r1.cost <= r0.cost
    with pytest.raises(RuntimeError):
        r0.improve(1.0)
    root = int(r1.table.path(r1.goal_id)[0][2])
    d = r1.table.download()
    g_root, s_root = float(d["g"][root]), d["state"][:, root].copy()
    env.editMap(w.walls["mid"], 100)
    r2 = r1.replan(advance=2)
    fresh = env.search(s_root, goal, eps=EPS, start_g=g_root, **kw)
    print(r0, r1, r2, fresh)
    assert r2.found and fresh.found and bits([r2.cost])[0] == bits([fresh.cost])[0]
    assert r2._params["eps"] == EPS and EPS != 3.0
    fresh.free()
    r2.free()
    env.close()


def test_improve_keeps_the_rules_of_a_timed_search(engine):
    m = engine
    env, start, goal = wall_env(m)
    other = env.search(goal, start, capacity=1 << 15, sight=False)
    p = other.path()
    avoid = env.alloc_reservations((p[0].reshape(-1, 1), p[1].reshape(-1, 1)), 0.5, n_steps=200, radius=0.3)
    other.free()
    kw = dict(capacity=1 << 16, sight=False, avoid=avoid, radius=0.3, wait=True)
    res = env.search(start, goal, eps=3.0, **kw)
    with pytest.raises(ValueError):
        res.improve(1.0)  # the search ran with avoid
    res = res.improve(1.0, avoid=avoid)
    fresh = env.search(start, goal, eps=1.0, **kw)
    print(res, fresh)
    assert res.found and fresh.found and abs(res.cost - fresh.cost) <= res.bound()["slack"]
    plain = env.search(start, goal, eps=3.0, capacity=1 << 15, sight=False)
    with pytest.raises(ValueError):
        plain.improve(1.0, avoid=avoid)  # ... and this one without
    for x in (plain, fresh, res, avoid):
        x.free()
    env.close()
