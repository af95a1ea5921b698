"""The timed shortcut, the timed smooth and refine_prioritised (include/mplx_reserve_poly.h, search.py) on the device.

Scenario: the pocket lane of tests/test_gpu_wait.py (one east-west lane with a side pocket two cells deep; robot 1 starts
at rest on the lane in robot 0's way, waits, ducks into the pocket and goes on) with a second, walled-off lane below it on
which robot 2 drives alone.  An UNTIMED shortcut of robot 1 hops along the lane past the pocket, where robot 0 drives:
that is the conflict the search paid waits and a detour to avoid, and the timed shortcut must not admit it.  The plan is
made once per module."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import reserve_poly_model as RPM
import shortcut_model as SHM
from test_gpu_solve import same_bits

pytestmark = pytest.mark.gpu

STEP, R = 0.25, 0.3
THREE = [-0.5, 0.0, 0.5]
_CACHE = {}


def lane_env(m, cells):
    env = m.EnvMap(2)
    env.setMap([0.0, 0.0], [cells.shape[1], cells.shape[0]], cells.ravel(), 1.0)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls(THREE, 2))
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    return env


def scenario(m):
    """env, plan (plan_prioritised, wait and park_goal, keep=True) of the three robots; kept for the module."""
    if "plan" not in _CACHE:
        cells = np.full((9, 25), 100, np.int8)  # [y][x]
        cells[3, :17] = 0
        cells[4:6, 9] = 0
        cells[7, :] = 0
        env = lane_env(m, cells)
        wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
        starts = np.stack([wp([1.5, 3.5]), wp([9.5, 3.5]), wp([23.5, 7.5])], axis=1)
        goals = np.stack([wp([15.5, 3.5]), wp([13.5, 3.5]), wp([1.5, 7.5])])
        plan = m.search.plan_prioritised(env, starts, goals, STEP, R, wait=True, park_goal=True, keep=True, capacity=1 << 17,
                                         max_frontier=4096, n_steps=int(60 / STEP), sight=False)
        assert plan["status"] == [m.search.FOUND] * 3 and not plan["conflicts"].charged.any()
        _CACHE["plan"] = (env, plan)
    return _CACHE["plan"]


def chain_states(env, path):
    """[4D+2][W][1]: the chain states of (start, actions)."""
    return np.ascontiguousarray(env.traj_info(path[0], path[1].reshape(-1, 1), want_states=True)["seg_state"][:, :len(path[1]) + 1, :1])


def table_of(env, plan, robots, t0=None, n_steps=None):
    """The reservation table a robot of lower priority sees: the raw chains of `robots`, PARK, group = the position."""
    H = max(len(plan["paths"][r][1]) for r in robots)
    st = np.stack([plan["paths"][r][0] for r in robots], axis=1)
    ac = np.full((H, len(robots)), -1, np.int32)
    for k, r in enumerate(robots):
        ac[:len(plan["paths"][r][1]), k] = plan["paths"][r][1]
    return env.alloc_reservations((st, ac), STEP, n_steps=plan["n_steps"] if n_steps is None else n_steps,
                                  t0=plan["t0"][robots] if t0 is None else t0, radius=R, park=True)


def pair_hits(env, sc, table, states, t0):
    """The model's hit of every pair problem of the shortcut `sc` ([W - 1][max_hop]), from the device's own samples of
    the pair set and the table's own positions; and t_start [P]."""
    pairs, W, hop = sc.pairs, states.shape[1], sc.max_hop
    t_i = states[-1, :, 0]
    ts = np.repeat(np.float64(t0) + t_i[:W - 1], hop)
    info = pairs.info()
    n = table.n_steps
    tl = np.arange(n)[None, :] * np.float64(STEP) - ts[:, None]
    pos = pairs.sample(times=np.ascontiguousarray(tl))["samples"][:2]
    hit, _, _ = RPM.check(info["status"], info["n_segs"], info["total_time"], ts, R, None, STEP, table.positions(),
                          lambda k, i, t: pos[:, k, i])
    return hit.reshape(W - 1, hop), ts


def same_shortcut(a, b, what):
    for key in ("status", "n_keep", "keep_rows"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), (what, key)
    for key in ("cost", "chain_cost", "edge_cost"):
        same_bits(getattr(a, key), getattr(b, key), "%s: %s" % (what, key))
    same_bits(a.pairs.coefficients(), b.pairs.coefficients(), what + ": pair coefficients")
    same_bits(a.pairs.dts(), b.pairs.dts(), what + ": pair durations")
    t = np.linspace(0.0, float(a.poly.total_time.max()), 33)
    same_bits(a.poly.sample(times=t)["samples"], b.poly.sample(times=t)["samples"], what + ": samples")
    assert np.array_equal(a.poly.n_segs, b.poly.n_segs)


def host_twin(m, env, states, hop, table=None):
    """mplx_shortcut / mplx_shortcut_timed with host pointers: (rows, chain_hit or None)."""
    A = m._abi
    F, W, Q = states.shape
    P = Q * (W - 1) * hop
    pairs, res = m.PolyTrajSet(env, P, 2), m.PolyTrajSet(env, Q, W)
    rows = {"status": np.zeros(Q, np.uint8), "n_keep": np.zeros(Q, np.int32), "keep": np.zeros((W, Q), np.int32), "cost": np.zeros(Q),
            "chain_cost": np.zeros(Q), "edge_cost": np.zeros((Q, W - 1, hop))}
    i, o = A.ShortcutIn(), A.ShortcutOut()
    i.states, i.n_query, i.w_max, i.control, i.stride, i.max_hop = states.ctypes.data, Q, W, int(m.ACC), Q, hop
    for k, v in rows.items():
        setattr(o, k, v.ctypes.data)
    o.keep_stride = Q
    ch = None
    if table is None:
        A.check(env._ctx, A.lib().mplx_shortcut(pairs._h, res._h, C.byref(i), C.byref(o)))
    else:
        ch = np.full(Q, 7, np.int64)
        A.check(env._ctx, A.lib().mplx_shortcut_timed(pairs._h, res._h, C.byref(i), C.byref(o), table._res, ch.ctypes.data))
    pairs.free()
    res.free()
    return rows, ch


def test_without_a_table_and_with_an_empty_one(engine):
    """avoid=None is the shortcut as it was (the device form and the host twin agree byte for byte, and
    tests/test_gpu_shortcut.py holds both to the model); an EMPTY table (a K == 0 fill) whose horizon holds the chain
    changes no bit of it and reports chain_hit -1; a horizon the chain leaves admits the chain's own edges only."""
    m = engine
    env, plan = scenario(m)
    states = chain_states(env, plan["paths"][1])
    W = states.shape[1]
    plain = env.shortcut(states)
    assert plain.chain_hit is None and plain.status[0] == 0 and plain.n_keep[0] < W
    rows, _ = host_twin(m, env, states, W - 1)
    for key in ("status", "n_keep", "cost", "chain_cost", "edge_cost"):
        same_bits(rows[key], getattr(plain, key), "host twin: " + key)
    assert np.array_equal(rows["keep"], plain.keep_rows)
    empty = env.alloc_reservations((np.zeros((env.n_fields, 0)), np.zeros((1, 0), np.int32)), STEP, n_steps=plan["n_steps"], radius=R)
    timed = env.shortcut(states, avoid=empty, t0=0.0, radius=R)
    same_shortcut(timed, plain, "empty table")
    assert timed.chain_hit.tolist() == [-1]
    rows_t, ch = host_twin(m, env, states, W - 1, empty)
    assert ch.tolist() == [-1] and np.array_equal(rows_t["keep"], plain.keep_rows)
    same_bits(rows_t["edge_cost"], plain.edge_cost, "timed host twin: edge_cost")
    # the chain ends at t = W - 1: a table of W - 1 seconds less one instant ends before it
    short = env.alloc_reservations((np.zeros((env.n_fields, 0)), np.zeros((1, 0), np.int32)), STEP, n_steps=int((W - 1) / STEP), radius=R)
    cut = env.shortcut(states, avoid=short, t0=0.0, radius=R)
    assert cut.chain_hit.tolist() == [-2] and cut.status[0] == 0
    assert cut.cost[0] >= plain.cost[0] and np.isinf(cut.edge_cost[0, 0, W - 2]) and np.isfinite(plain.edge_cost[0, :, 0]).all()
    with pytest.raises(ValueError):
        env.shortcut(states, t0=0.0)
    # two queries were set, the shortcut has one
    empty.set_queries([0.0, 0.0], R)
    d_states = m.DeviceArray(env, states.nbytes)
    d_states.upload(states)
    pr, rs = m.PolyTrajSet(env, (W - 1) * (W - 1), 2), m.PolyTrajSet(env, 1, W)
    i, o = m._abi.ShortcutIn(), m._abi.ShortcutOut()
    i.states, i.n_query, i.w_max, i.control, i.stride, i.max_hop = d_states.ptr, 1, W, int(m.ACC), 1, W - 1
    with pytest.raises(m._abi.MplxError) as e:
        m._abi.check(env._ctx, m._abi.lib().mplx_shortcut_timed_device(pr._h, rs._h, C.byref(i), C.byref(o), empty._res, None))
    assert e.value.code == m._abi.ERR_ARG
    with pytest.raises(m._abi.MplxError) as e:
        m._abi.check(env._ctx, m._abi.lib().mplx_shortcut_timed_device(pr._h, rs._h, C.byref(i), C.byref(o), None, None))
    assert e.value.code == m._abi.ERR_ARG
    for x in (pr, rs, d_states):
        x.free()
    for x in (plain, timed, cut, empty, short):
        x.free()


def test_a_chain_with_waits(engine):
    """Robot 1's chain has waits.  Precondition: its UNTIMED shortcut conflicts with robot 0 (conflicts on the merged
    set charges it).  The timed shortcut, against robot 0's reservation, has no conflict; its cost lies between the
    untimed cost and chain_cost; its pair hits equal the model's, and every kept hop is the choice of the programme
    (shortcut_model.dp) on the cost matrix masked with them."""
    m = engine
    env, plan = scenario(m)
    p1 = plan["paths"][1]
    states = chain_states(env, p1)
    W = states.shape[1]
    assert int(np.sum(np.all(states[:4, 1:, 0] == states[:4, :-1, 0], axis=0))) >= 1, "robot 1 does not wait"
    with pytest.raises(ValueError):  # the search ran with avoid
        plan["results"][1].shortcut()
    table = table_of(env, plan, [0])
    untimed = env.shortcut(states)
    timed = plan["results"][1].shortcut(avoid=table)
    assert untimed.status[0] == 0 and timed.status[0] == 0 and timed.chain_hit.tolist() == [-1]
    raw0 = env.shortcut(chain_states(env, plan["paths"][0]), max_hop=1)

    def charged(sc):
        both = m.search.load_traj_rows(env, [raw0.segments(0), sc.segments(0)])
        res = both.conflicts(STEP, plan["n_steps"], t0=plan["t0"][[0, 1]], radius=R, park=True)
        both.free()
        return res

    cu, ct = charged(untimed), charged(timed)
    print("untimed: cost %.3f keep %s first_step %s; timed: cost %.3f keep %s; chain %.3f" % (
        untimed.cost[0], untimed.keep[0].tolist(), cu.first_step.tolist(), timed.cost[0], timed.keep[0].tolist(), timed.chain_cost[0]))
    assert cu.charged.any(), "the untimed shortcut of the chain with waits does not conflict: the scenario shows nothing"
    assert not ct.charged.any()
    assert untimed.cost[0] <= timed.cost[0] <= timed.chain_cost[0] and untimed.cost[0] < timed.cost[0]
    same_bits(timed.chain_cost, untimed.chain_cost, "chain_cost")
    # the model: the pair hits, then the programme on the masked matrix
    hit, ts = pair_hits(env, timed, table, states, plan["t0"][1])
    got = table.check_poly(timed.pairs, ts, R)
    assert np.array_equal(got["hit"].reshape(W - 1, W - 1), hit)
    assert (hit[:, 1:] >= 0).any() and (hit[:, 0] == -1).all()
    masked = RPM.admit(untimed.edge_cost[0], hit)
    same_bits(timed.edge_cost[0], masked, "masked edge costs")
    st, keep, cost, chain = SHM.dp(masked, W, W - 1)
    assert st == 0 and timed.keep[0].tolist() == keep
    same_bits(timed.cost, [cost], "cost of the programme")
    for x in (untimed, timed, raw0, table):
        x.free()


def test_a_rest_pair(engine):
    """A two-state chain p -> p over dt: the constant polynomial, cost w dt, with a table and without."""
    m = engine
    env, plan = scenario(m)
    dt = 3.0
    states = np.zeros((env.n_fields, 2, 1))
    states[:2, :, 0] = np.array([[9.5, 9.5], [4.5, 4.5]])
    states[-1, 1, 0] = dt
    table = table_of(env, plan, [0])
    for sc in (env.shortcut(states), env.shortcut(states, avoid=table, t0=2.0, radius=R)):
        assert sc.status[0] == 0 and sc.keep[0].tolist() == [0, 1]
        coef = sc.pairs.coefficients()[0, :, :, 0]
        assert np.array_equal(coef[0], [9.5, 4.5]) and (coef[1:] == 0.0).all(), coef
        same_bits(sc.cost, [np.float64(env._p.w) * np.float64(dt)], "cost of a rest pair")
        s = sc.poly.sample(times=np.array([0.0, 0.7, 1.5, 3.0]))["samples"]
        assert (s[0, 0] == 9.5).all() and (s[1, 0] == 4.5).all() and (s[2:4, 0] == 0.0).all()
        if sc.chain_hit is not None:
            assert sc.chain_hit.tolist() == [-1]  # in the pocket while robot 0 passes
        sc.free()
    table.free()


def test_a_stale_chain_is_reported(engine):
    """Against a table refilled with robot 0 DELAYED, robot 1's own chain no longer holds: chain_hit names the first
    adjacent edge in conflict (the smallest hit of the model over the chain's own pairs); the trajectory returned is
    still made of admitted edges (the chain's own stay admitted) and every hop it keeps is clear."""
    m = engine
    env, plan = scenario(m)
    states = chain_states(env, plan["paths"][1])
    W = states.shape[1]
    found = None
    for delay in (2.0, 1.0, 3.0, 4.0, 5.0, 6.0):
        table = table_of(env, plan, [0], t0=np.array([delay]))
        sc = plan["results"][1].shortcut(avoid=table)
        if sc.chain_hit[0] >= 0:
            found = (delay, table, sc)
            break
        sc.free()
        table.free()
    assert found is not None, "no delay of robot 0 makes robot 1's chain stale"
    delay, table, sc = found
    hit, _ = pair_hits(env, sc, table, states, plan["t0"][1])
    assert sc.chain_hit[0] == RPM.chain_hit(hit, W) == hit[:, 0][hit[:, 0] >= 0].min()
    print("robot 0 delayed by %.1f: chain_hit instant %d partner %d" % (delay, sc.chain_hit[0] >> 32, sc.chain_hit[0] & 0xffffffff))
    assert sc.status[0] == 0 and np.isfinite(sc.cost[0]) and sc.keep[0][0] == 0 and sc.keep[0][-1] == W - 1
    for i, j in zip(sc.keep[0][:-1], sc.keep[0][1:]):
        assert j == i + 1 or hit[i, j - i - 1] == -1
    sc.free()
    table.free()


def test_smooth_timed(engine):
    """smooth(timed=True) of the chain with waits: solved, the segment times are the chain's own differences bit for
    bit, the samples at the chain times are the chain states (positions; to 1e-10: a quintic with coefficients of order 10
    evaluated at the end of a segment of a few seconds, each term rounded at 2^-53 relative), and reserve_hit is
    check_poly of the same set.  v other than the default, or avoid without timed, raises."""
    m = engine
    env, plan = scenario(m)
    r1 = plan["results"][1]
    table = table_of(env, plan, [0])
    states = chain_states(env, plan["paths"][1])
    W = states.shape[1]
    with pytest.raises(ValueError):
        r1.smooth(v=[1.0, 2.0], timed=True)
    with pytest.raises(ValueError):
        r1.smooth(avoid=table)
    poly = r1.smooth(timed=True, avoid=table)
    assert poly.status.tolist() == [0] and poly.n_segs.tolist() == [W - 1]
    t = states[-1, :, 0]
    same_bits(poly.dts()[:, 0], t[1:] - t[:-1], "segment times")
    same_bits(poly.chain_times[:, 0], t, "chain times")
    s = poly.sample(times=np.ascontiguousarray(t))["samples"]
    assert np.abs(s[:2, 0, :] - states[:2, :, 0]).max() <= 1e-10, np.abs(s[:2, 0, :] - states[:2, :, 0]).max()
    again = table.check_poly(poly, plan["t0"][1], R, -1)
    assert np.array_equal(poly.reserve_hit["hit"], again["hit"]) and poly.reserve_hit["n_hit"] == again["n_hit"]
    print("smooth(timed=True): hit", poly.reserve_hit["hit"].tolist())
    plain = r1.smooth(timed=True)
    assert plain.reserve_hit is None
    same_bits(plain.coefficients(), poly.coefficients(), "coefficients with and without avoid")
    for x in (poly, plain, table):
        x.free()


def test_refine_prioritised(engine):
    """The three robots: the final conflicts charges nobody, every cost is <= its raw cost, robots 0 and 1 are
    refined.  Robot 2, alone on its lane, is ARRANGED to get a chain hit: the table's horizon is cut to end before its
    chain does (-2), so it keeps its raw chain and is reported."""
    m = engine
    env, plan = scenario(m)
    lens = [len(p[1]) for p in plan["paths"]]
    assert lens[2] > max(lens[0], lens[1]), lens  # (the horizon can be cut for robot 2 alone)
    full = m.search.refine_prioritised(env, plan, STEP)
    print("refine:", full["cost_before"], full["cost_after"], full["chain_hit"], full["refined"])
    assert full["chain_hit"].tolist() == [-1, -1, -1] and full["refined"].all()
    assert not full["conflicts"].charged.any()
    assert (full["cost_after"] <= full["cost_before"]).all() and (full["cost_after"] < full["cost_before"]).any()
    full["trajs"].free()
    cut = dict(plan, n_steps=int(max(lens[0], lens[1]) / STEP) + 1)
    out = m.search.refine_prioritised(env, cut, STEP)
    print("refine, short horizon:", out["cost_before"], out["cost_after"], out["chain_hit"], out["refined"])
    assert out["chain_hit"].tolist() == [-1, -1, -2] and out["refined"].tolist() == [True, True, False]
    assert out["cost_after"][2] == out["cost_before"][2] and (out["cost_after"] <= out["cost_before"]).all()
    assert not out["conflicts"].charged.any()
    raw2 = env.shortcut(chain_states(env, plan["paths"][2]), max_hop=1)
    t = np.linspace(0.0, float(lens[2]), 41)
    same_bits(out["trajs"].sample(times=t)["samples"][:, 2], raw2.poly.sample(times=t)["samples"][:, 0], "robot 2 keeps its raw chain")
    raw2.free()
    out["trajs"].free()
