"""GPU: OpenSet.set_heur("robust") (include/mplx_heur.h) -- the pushes of an open set against tests/heur_model.py's
HeurOpenModel / HeurMultiOpenModel, f and flags bit for bit: open and closed, with sight, three queries whose goals and
goal controls differ, a goal field under it (the larger of the two, +inf kept), priors in either order, and the reset to
the default against an open set that never had the mode."""
import numpy as np
import pytest

import field_model as FM
import heur_model as HM
import open_model as OM
from test_gpu_field import map_env, push_world

pytestmark = pytest.mark.gpu

POISON = 0xAB
N_ROWS = 300
W, VMAX = 1.0, 2.0


def code(m, fn):
    with pytest.raises(m._abi.MplxError) as e:
        fn()
    return e.value.code


class TableStub:
    """What the open models read of a table: the device table's own hashes, the queries, the node count."""

    def __init__(self, hashes, query, Q):
        self.hash, self.query, self.n_nodes, self.n_queries = hashes, query, len(hashes), Q


def rows_of(D, dims, res, goals, n_fields, order, yaw, seed):
    """N_ROWS state columns on a 0.25 lattice across the map with live rows up to `order`, and per query: the goal's own
    state, two rows inside its box, a row on its position with a live velocity (dp = 0), a row off the map and a row with
    a NaN velocity (ignored under ROBUST)."""
    rng = np.random.default_rng(seed)
    Q = len(goals)
    s = np.zeros((n_fields, N_ROWS))
    for i in range(D):
        s[i] = rng.integers(1, int(dims[i] * res * 4), N_ROWS) / 4.0 + 0.01 * rng.integers(0, 3, N_ROWS)
    if order >= 2:
        s[D:2 * D] = rng.integers(-4, 5, (D, N_ROWS)) / 4.0
    if order >= 3:
        s[2 * D:3 * D] = rng.integers(-4, 5, (D, N_ROWS)) / 4.0
    if yaw:
        s[4 * D] = rng.integers(-3, 4, N_ROWS) * 0.1
    query = (np.arange(N_ROWS) % Q).astype(np.int32)
    for q in range(Q):
        k = 10 * q + Q  # (k % Q == q)
        cols = [k, k + Q * 1, k + Q * 2, k + Q * 3, k + Q * 4, k + Q * 5]
        assert all(query[c] == q for c in cols)
        s[:, cols[0]] = goals[q]
        s[:, cols[1]] = goals[q]
        s[:D, cols[1]] += 0.2
        s[:, cols[2]] = goals[q]
        s[:D, cols[2]] -= 0.3
        s[D:2 * D, cols[2]] = 0.0 if order < 2 else 0.5
        s[:D, cols[3]] = goals[q][:D]
        s[0, cols[4]] = -0.75
        s[D, cols[5]] = np.nan
    return make_distinct(s, query, D, {1: HM.VEL, 2: HM.ACC, 3: HM.JRK}[order] | (HM.YAW if yaw else 0)), query


def make_distinct(s, query, D, control):
    """The seeds must be distinct nodes: waypoint.h's hash collides for some small lattice states, so a column whose
    (query, hash) is taken moves on by a quarter along y."""
    from prior_model import lattice_hash
    taken = set()
    for k in range(N_ROWS):
        if np.isnan(s[D, k]):
            continue
        while (int(query[k]), lattice_hash(D, control, [float(x) for x in s[:, k]])) in taken:
            s[1, k] += 0.25
        taken.add((int(query[k]), lattice_hash(D, control, [float(x) for x in s[:, k]])))
    return s


CASES = [(2, "ACC", 1, [0]), (2, "ACC", 3, [0, "VEL", "ACC"]), (3, "JRK", 3, [0, "ACC", "VEL"]), (3, "ACCxYAW", 1, [0]),
         (2, "VEL", 1, [0])]


@pytest.mark.parametrize("D,control,Q,goal_controls", CASES, ids=["%dd-%s-Q%d" % c[:3] for c in CASES])
def test_push_with_robust_equals_the_model(engine, D, control, Q, goal_controls):
    m = engine
    A = m._abi
    yaw = control.endswith("YAW")
    order = {"VEL": 1, "ACC": 2, "JRK": 3}[control.replace("xYAW", "")]
    ctl = getattr(m, control)
    gcs = [getattr(m, g) if g else 0 for g in goal_controls]
    dims, res, cells = push_world(D)
    env = map_env(m, dims, cells, res=res, control=ctl, vals=(-0.5, 0.0, 0.5), v_max=VMAX, yaw=yaw)
    F = env.n_fields
    org = [0.0] * D
    goal_pos = [[(dims[0] - 3 + 0.5) * res] + [1.5 * res] * (D - 1), [(dims[0] - 2 + 0.5) * res] + [2.5 * res] * (D - 1),
                [(dims[0] - 3 + 0.5) * res] + [3.5 * res] * (D - 1)][:Q]
    goals = np.zeros((Q, F))
    goals[:, :D] = goal_pos
    if order >= 2:
        goals[:, D] = [0.5, 0.0, -0.25][:Q]  # goals that move
    states, query = rows_of(D, dims, res, goals, F, order, yaw, 17 * D + Q)
    n = N_ROWS
    g = 0.25 * (np.arange(n) % 16)
    tab = env.alloc_table(1024, n_queries=Q)
    opn = env.alloc_open(tab)
    if Q > 1:
        opn.set_goals(goals, w=W, v_max=VMAX, tol_pos=0.5, goal_control=gcs)
    else:
        env.set_goal(goals[0], w=W, v_max=VMAX, tol_pos=0.5, goal_control=gcs[0])
    fr = m.TableFrontier(env, n)
    assert tab.seed(states, g, frontier=fr, query=query if Q > 1 else None) == n  # node k = seed k (the states are distinct)
    d = tab.download()
    frd = fr.download()
    assert d["n_nodes"] == n and np.array_equal(frd["id"], np.arange(n))
    from prior_model import lattice_hash
    goal_hash = [lattice_hash(D, gcs[q] if gcs[q] else ctl, [float(x) for x in goals[q]]) for q in range(Q)]
    stub = TableStub(d["hash"], query, Q)
    blocked = [OM.ray_blocked(cells, dims, org, res, goals[q][:D]) for q in range(Q)]
    kw = dict(tol_pos=0.5)

    def models():
        if Q > 1:
            import multi_model as MM
            return (MM.MultiOpenModel(stub, D, goals, goal_hash, W, VMAX, blocked=blocked, **kw),
                    HM.HeurMultiOpenModel(stub, D, goals, goal_hash, W, VMAX, blocked=blocked, control=ctl, goal_controls=gcs, **kw))
        return (OM.OpenModel(stub, D, goals[0], goal_hash[0], W, VMAX, blocked=blocked[0], **kw),
                HM.HeurOpenModel(stub, D, goals[0], goal_hash[0], W, VMAX, blocked=blocked[0], control=ctl, goal_control=gcs[0], **kw))

    cap = opn.capacity
    v = opn.view()

    def pushed(o, eps, sight, closed, n_max):
        o.clear()
        env.synchronize()
        vv = o.view()
        A.check(env._ctx, A.lib().mplx_memset(env._ctx, vv.f, POISON, cap * 8))
        A.check(env._ctx, A.lib().mplx_memset(env._ctx, vv.flags, POISON, cap))
        o.push(fr, n_max=n_max, eps=eps, sight=sight, closed=closed)
        env.synchronize()
        return tab._read(vv.f, np.uint64, cap), tab._read(vv.flags, np.uint8, cap)

    def expect(model, eps, sight, closed, n_max):
        model.f, model.flags = {}, {}
        model.push(frd, n_max, eps, sight)
        f = np.full(cap, np.frombuffer(bytes([POISON] * 8), np.uint64)[0], np.uint64)
        fl = np.full(cap, POISON, np.uint8)
        for i, x in model.f.items():
            f[i] = np.float64(x).view(np.uint64)
        for i, x in model.flags.items():
            fl[i] = (x & ~OM.IS_OPEN) if closed else x
        return f, fl

    fresh_tab = env.alloc_table(1024, n_queries=Q)  # an open set that never has the mode
    fresh = env.alloc_open(fresh_tab)
    if Q > 1:
        fresh.set_goals(goals, w=W, v_max=VMAX, tol_pos=0.5, goal_control=gcs)
    ffr = m.TableFrontier(env, n)
    assert fresh_tab.seed(states, g, frontier=ffr, query=query if Q > 1 else None) == n
    ffr.free()

    differ = ignored = goal_rows = 0
    for (eps, sight, closed), n_max in zip(((1.0, False, False), (2.0, False, True), (1.0, True, False), (0.5, True, True)), (n, 65, 64, 1)):
        plain, robust = models()
        what = "eps %r sight %r closed %r n_max %d" % (eps, sight, closed, n_max)
        f0, fl0 = pushed(opn, eps, sight, closed, n_max)
        opn.set_heur("robust")
        f1, fl1 = pushed(opn, eps, sight, closed, n_max)
        opn.clear()  # keeps the mode
        f1b, fl1b = pushed(opn, eps, sight, closed, n_max)
        opn.set_heur(None)
        f2, fl2 = pushed(opn, eps, sight, closed, n_max)
        f3, fl3 = pushed(fresh, eps, sight, closed, n_max)
        w0, wl0 = expect(plain, eps, sight, closed, n_max)
        w1, wl1 = expect(robust, eps, sight, closed, n_max)
        assert np.array_equal(f0, w0) and np.array_equal(fl0, wl0), what      # the model knows the plain push
        assert np.array_equal(f1, w1) and np.array_equal(fl1, wl1), what
        assert np.array_equal(f1b, f1) and np.array_equal(fl1b, fl1), what
        assert np.array_equal(f2, f0) and np.array_equal(fl2, fl0), what      # reset: the plain push again ...
        assert np.array_equal(f3, f0) and np.array_equal(fl3, fl0), what      # ... that of an open set that never had the mode
        pushed0, pushed1 = fl0[:n_max] != POISON, fl1[:n_max] != POISON
        assert np.all(f1[:n_max][pushed1].view(np.float64) >= f0[:n_max][pushed1].view(np.float64)), what  # never below the default
        if n_max == n:
            differ = int(np.sum(f1[:n][pushed1] != f0[:n][pushed1]))
            ignored = int(np.sum(pushed0 & ~pushed1))
            goal_rows = int(np.sum(fl1[:n][pushed1] & OM.IS_GOAL))
    print(control, D, Q, "keys above the default:", differ, "rows ignored for a NaN:", ignored, "goal-region rows:", goal_rows)
    assert differ > n // 2 and ignored == Q and goal_rows >= 1
    for b in (fresh, fresh_tab, fr, opn, tab):
        b.free()
    env.close()


@pytest.mark.parametrize("D,Q", [(2, 1), (2, 3)])
def test_push_with_robust_and_a_field(engine, D, Q):
    """h = max(ROBUST, the field's h); +inf where no chain leaves the cell; a NaN row is ignored."""
    m = engine
    dims, res, cells = push_world(D)
    VMAX = 1.0  # (a slow robot: the detour round the wall outweighs the effort of the straight connection)
    env = map_env(m, dims, cells, res=res, control=m.ACC, vals=(-0.5, 0.0, 0.5), v_max=VMAX)
    F = env.n_fields
    org = [0.0] * D
    goal_pos = [[(dims[0] - 3 + 0.5) * res] + [1.5 * res] * (D - 1), [(dims[0] - 2 + 0.5) * res] + [2.5 * res] * (D - 1),
                [(dims[0] - 3 + 0.5) * res] + [3.5 * res] * (D - 1)][:Q]
    goals = np.zeros((Q, F))
    goals[:, :D] = goal_pos
    foq = [0, -1, 1][:Q]
    fgoals = goals[[0, 2]] if Q == 3 else goals[[0]]
    fld = env.alloc_field().build(fgoals, 0.5)
    dist = fld.dist()
    states, query = rows_of(D, dims, res, goals, F, 2, False, 5 + Q)
    # rows at rest far behind the wall (the field's bound wins there) and the sealed pocket (+inf)
    for j in range(40, 80):
        states[D:2 * D, j] = 0.0
        states[0, j] = 0.25 + 0.25 * (j % 8)
    states[:D, 81] = (2 + 0.5) * res
    states = make_distinct(states, query, D, m.ACC)
    n = N_ROWS
    g = 0.25 * (np.arange(n) % 16)
    tab = env.alloc_table(1024, n_queries=Q)
    opn = env.alloc_open(tab)
    if Q > 1:
        opn.set_goals(goals, w=W, v_max=VMAX, tol_pos=0.5)
    else:
        env.set_goal(goals[0], w=W, v_max=VMAX, tol_pos=0.5)
    fr = m.TableFrontier(env, n)
    assert tab.seed(states, g, frontier=fr, query=query if Q > 1 else None) == n
    d = tab.download()
    from prior_model import lattice_hash
    goal_hash = [lattice_hash(D, m.ACC, [float(x) for x in goals[q]]) for q in range(Q)]
    kinds = {"field": 0, "robust": 0, "inf": 0, "nan": 0, "goal": 0}
    want = np.full(n, np.nan)
    for k in range(n):
        q = int(query[k])
        is_goal = int(d["hash"][k]) == goal_hash[q]
        h_dyn = 0.0 if is_goal else float(HM.robust(states[:, [k]], goals[q], m.ACC, 0, W, VMAX, D)[0])
        if foq[q] >= 0:
            h_fld = float(FM.heuristic(states[:D, k], goals[q], W, VMAX, dist[foq[q]], dims, org, res, is_goal)[0])
        else:
            h_fld = float(FM.default_heuristic(states[:D, k], goals[q], W, VMAX, D, is_goal))
        h = h_fld if h_dyn <= h_fld else h_dyn
        kinds["goal" if is_goal else "nan" if h != h else "inf" if h == np.inf else "field" if h_fld > h_dyn else "robust"] += 1
        key = FM.key(g[k], 1.0, h)
        if key is not None:
            want[k] = key
    print("field + robust", D, Q, kinds)
    assert kinds["field"] >= 10 and kinds["robust"] >= n // 4 and kinds["inf"] >= 1 and kinds["nan"] == Q and kinds["goal"] == Q
    opn.set_field(fld, foq)
    opn.set_heur("robust")
    for closed in (False, True):
        opn.clear()
        opn.push(fr, n_max=n, eps=1.0, closed=closed)
        env.synchronize()
        got = opn.download()
        seen = (got["flags"][:n] & OM.SEEN) != 0
        assert np.array_equal(seen, ~np.isnan(want))
        assert np.array_equal(got["f"][:n][seen].view(np.uint64), want[seen].view(np.uint64))
        assert np.all(((got["flags"][:n][seen] & OM.IS_OPEN) != 0) == (not closed))
    for b in (fr, opn, tab, fld):
        b.free()
    env.close()


def test_robust_and_priors_exclude_each_other(engine):
    m = engine
    A = m._abi
    dims, res, cells = push_world(2)
    env = map_env(m, dims, cells, res=res, control=m.ACC, vals=(-0.5, 0.0, 0.5), v_max=VMAX)
    F = env.n_fields
    goal = np.zeros(F)
    goal[:2] = [8.25, 0.75]
    st = np.zeros((F, 1))
    st[:2, 0] = [1.25, 5.25]
    U = np.asarray(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    tab = env.alloc_table(64)
    opn = env.alloc_open(tab)
    assert code(m, lambda: opn.set_heur("reference")) == A.ERR_ARG            # host only
    assert code(m, lambda: opn.set_heur(9)) == A.ERR_ARG
    opn.set_goals(goal.reshape(1, -1), tol_pos=0.5, w=0.0)
    assert code(m, lambda: opn.set_heur("robust")) == A.ERR_ARG               # w <= 0 where the mode is set
    opn.set_goals(goal.reshape(1, -1), tol_pos=0.5, w=W)
    opn.set_heur("robust")
    assert code(m, lambda: opn.set_priors(st, np.array([[4], [4]], np.int32), m.ACC, U, 1.0)) == A.ERR_STATE
    opn.set_heur(None)
    opn.set_priors(st, np.array([[4], [4]], np.int32), m.ACC, U, 1.0)
    assert code(m, lambda: opn.set_heur("robust")) == A.ERR_STATE
    opn.clear_priors()
    opn.set_heur("robust")
    # a goal whose w is not positive, set after the mode: the push refuses
    opn.set_goals(goal.reshape(1, -1), tol_pos=0.5, w=0.0)
    fr = m.TableFrontier(env, 1)
    assert tab.seed(st, frontier=fr) == 1
    assert code(m, lambda: opn.push(fr, n_max=1)) == A.ERR_STATE
    with pytest.raises(ValueError):
        env.search(st[:, 0], goal, heur="robust", prior=m.search.Prior(st[:, 0], [4], m.ACC, U, 1.0))
    assert A.lib().mplx_open_set_heur(None, 2) == A.ERR_ARG
    for b in (fr, opn, tab):
        b.free()
    env.close()
