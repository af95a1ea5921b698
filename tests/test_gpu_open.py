"""GPU: the open set of include/mplx_open.h against tests/open_model.py.  Every comparison with the model is bit for bit:
f and flags of every node, every frontier row a select emits (ids, order, g, state rows, count) and the result.  The
searches are fed with the device's own lists, as tests/test_gpu_table.py feeds its sweeps."""
import ctypes as C
import math

import numpy as np
import pytest

import control_matrix as CM
import open_model as OM
from helpers import engine_env, oracle_env
from table_model import TableModel, oracle_provider, sweep
from test_gpu_parity import _small_world
from test_gpu_table import assert_frontier_equal, assert_table_equal, bits
from test_open import blocked_goal_cells, corridor_search, corridor_setup, hand_model
from test_plan_known_answer import corridor
from test_table import small_start

pytestmark = pytest.mark.gpu

PAT_I, PAT_D = 0x5A5A5A5A, -1234.5


def assert_open_equal(opn, model, what=""):
    got = opn.download()
    f, fl = model.arrays()
    assert got["n_nodes"] == model.table.n_nodes, what
    assert np.array_equal(got["flags"], fl), what + ": flags"
    seen = (fl & OM.SEEN) > 0
    assert np.array_equal(bits(got["f"][seen]), bits(f[seen])), what + ": f"


def assert_result_equal(got, want, what=""):
    for k in ("status", "goal_id", "count", "n_open"):
        assert got[k] == want[k], "%s: %s %r != %r" % (what, k, got[k], want[k])
    for k in ("f_min", "goal_f", "goal_g"):
        assert bits([got[k]])[0] == bits([want[k]])[0], "%s: %s %r != %r" % (what, k, got[k], want[k])


def patterned_frontier(m, env, capacity, spare):
    fr = m.TableFrontier(env, capacity, spare)
    n = fr.state_stride
    fr.id.upload(np.full(n, PAT_I, np.int32))
    fr.g.upload(np.full(n, PAT_D))
    fr.state.upload(np.full((fr.n_fields, n), PAT_D))
    return fr


def assert_spare_untouched(fr, what=""):
    n, cap = fr.state_stride, fr.capacity
    assert np.all(fr.id.download(np.int32, (n,))[cap:] == PAT_I), what
    assert np.all(fr.g.download(np.float64, (n,))[cap:] == PAT_D), what
    assert np.all(fr.state.download(np.float64, (fr.n_fields, n))[:, cap:] == PAT_D), what


def upload_frontier(m, env, host, capacity, count=None):
    """A device frontier of `capacity` holding the rows of `host`; rows past the capacity go into the spare entries."""
    n = len(host["id"])
    fr = m.TableFrontier(env, capacity, spare=max(n - capacity, 0))
    ids, g, st = np.zeros(fr.state_stride, np.int32), np.zeros(fr.state_stride), np.zeros((fr.n_fields, fr.state_stride))
    ids[:n], g[:n], st[:, :n] = host["id"], host["g"], host["state"]
    fr.id.upload(ids)
    fr.g.upload(g)
    fr.state.upload(st)
    fr.count.upload(np.array([host["count"] if count is None else count], np.int64))
    return fr


def select_both(opn, model, delta, fr, what=""):
    got = opn.select(delta, fr)
    want, want_fr = model.select(delta, fr.capacity)
    assert_result_equal(got, want, what)
    assert_frontier_equal(fr.download(), want_fr, what)
    return got, want_fr


def rest_env(m, with_map=False):
    """2D ACC at rest states: parameters and controls (a seed needs them), no map unless asked for."""
    env = m.EnvMap(2)
    if with_map:
        env.setMap([0.0, 0.0], [100, 50], np.zeros(5000, np.int8), 0.1)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-1.0, 0.0, 1.0], 2))
    env.set_v_max(OM.HAND_VMAX)
    env.set_dt(1.0)
    env.set_w(OM.HAND_W)
    return env


def test_hand_built_push_and_select(engine, oracle_lib):
    """tests/open_model.py::hand_scenario (its properties: tests/test_open.py): 5 000 nodes, a full tile of 4 096 ids and a
    partial one; rows that must be ignored and rows behind n_max / the capacity; selects with delta in {0, 2.5, 40,
    +inf} into capacities {0, 16, 5000} with spare entries; a second push that re-opens and re-keys; then selects until
    FOUND by the smallest id among the tied goal nodes."""
    m = engine
    table, model, states, goal, in_goal, ignored, push1, push2 = hand_model(oracle_lib)
    env = rest_env(m)
    env.set_goal(goal, tol_pos=OM.HAND_TOL)
    tab = env.alloc_table(OM.HAND_N + 100)
    seeds = m.TableFrontier(env, OM.HAND_N)
    assert tab.seed(states, frontier=seeds) == OM.HAND_N
    assert_table_equal(tab, table)
    opn = env.alloc_open(tab)
    assert_open_equal(opn, model, "a new open set")
    # push 1: n_max cuts the tail off
    host = OM.hand_frontier(states, push1, with_tail=True)
    fr1 = upload_frontier(m, env, host, len(host["id"]))
    opn.push(fr1, n_max=len(push1["id"]), eps=1.0)
    model.push(host, len(push1["id"]), 1.0)
    assert_open_equal(opn, model, "push 1")
    d_res = m.DeviceArray(env, 48)
    frs = {cap: patterned_frontier(m, env, cap, 64) for cap in (0, 16, 5000)}
    for delta, cap in OM.HAND_SELECTS:
        what = "select(%r, %d)" % (delta, cap)
        got = opn.select(delta, frs[cap], d_result=d_res)
        want, want_fr = model.select(delta, cap)
        assert_result_equal(got, want, what)
        assert_frontier_equal(frs[cap].download(), want_fr, what)
        assert_spare_untouched(frs[cap], what)
        assert_open_equal(opn, model, what)
        r = m._abi.OpenResult.from_buffer_copy(d_res.download(np.uint8, (48,)).tobytes())
        assert (r.status, r.goal_id, r.count, r.n_open) == (got["status"], got["goal_id"], got["count"], got["n_open"])
        assert bits([r.f_min, r.goal_f, r.goal_g]).tolist() == bits([got["f_min"], got["goal_f"], got["goal_g"]]).tolist()
    # push 2: the capacity cuts the tail off (the count on the device and n_max are larger)
    host = OM.hand_frontier(states, push2, with_tail=True)
    fr2 = upload_frontier(m, env, host, len(push2["id"]))
    opn.push(fr2, n_max=10 ** 9, eps=1.0)
    model.push(host, 10 ** 9, 1.0, capacity=len(push2["id"]))
    assert_open_equal(opn, model, "push 2")
    for k in range(200):
        got, _ = select_both(opn, model, 2.5, frs[5000], "select %d after push 2" % k)
        if got["status"] != OM.SELECTED:
            break
    assert got["status"] == OM.FOUND and got["n_open"] > 0 and got["count"] == 0
    assert_open_equal(opn, model, "FOUND")
    assert_spare_untouched(frs[5000])
    # clear: nothing open
    opn.clear()
    model.f, model.flags = {}, {}
    got, _ = select_both(opn, model, 0.0, frs[16], "after clear")
    assert got["status"] == OM.EMPTY and got["f_min"] == math.inf and got["goal_id"] == -1
    # eps = 0: f = g
    opn.push(fr2, n_max=100, eps=0.0)
    model.push(host, 100, 0.0)
    assert_open_equal(opn, model, "eps = 0")
    for b in [seeds, fr1, fr2, d_res] + list(frs.values()):
        b.free()
    opn.free()
    tab.free()
    env.close()


def test_single_node_and_nothing_open(engine, oracle_lib):
    m, O = engine, oracle_lib
    env = rest_env(m)
    goal = np.zeros(10)
    goal[:2] = OM.HAND_GOAL
    env.set_goal(goal, tol_pos=OM.HAND_TOL)
    start = np.zeros(10)
    start[:2] = [7.0, 1.0]
    tab = env.alloc_table(8)
    opn = env.alloc_open(tab)
    table = TableModel(10)
    model = OM.OpenModel(table, 2, goal, O.lattice_hash(2, O.ACC, goal), OM.HAND_W, OM.HAND_VMAX, tol_pos=OM.HAND_TOL)
    sel, one = patterned_frontier(m, env, 4, 8), m.TableFrontier(env, 1)
    # a table without nodes: push is a no-op, select is EMPTY
    one.count.upload(np.array([1], np.int64))
    one.id.upload(np.array([0], np.int32))
    opn.push(one, n_max=1, eps=1.0)
    opn.push(one, n_max=0, eps=1.0)
    got, _ = select_both(opn, model, 0.0, sel, "no nodes")
    assert got["status"] == OM.EMPTY
    # nodes, none pushed
    assert tab.seed(start, frontier=one) == 1
    want_seed, _ = table.seed(start, [O.lattice_hash(2, O.ACC, start)])
    got, _ = select_both(opn, model, 0.0, sel, "nothing pushed")
    assert got["status"] == OM.EMPTY
    # the single node: selected, then nothing is left
    opn.push(one, n_max=1, eps=1.0)
    model.push(want_seed, 1, 1.0)
    got, _ = select_both(opn, model, 0.0, sel, "one node")
    assert got["status"] == OM.SELECTED and got["count"] == 1 and got["n_open"] == 0 and got["f_min"] == 40.0
    got, _ = select_both(opn, model, 0.0, sel, "closed")
    assert got["status"] == OM.EMPTY
    assert_open_equal(opn, model)
    assert_spare_untouched(sel)
    for b in (sel, one):
        b.free()
    opn.free()
    tab.free()
    env.close()


def device_search(m, env, table, model, start, h0, eps, delta, cap, g_max, sight, max_rounds):
    """The loop of EnvMap.search spelled out, every step compared with the model fed with the device's own lists.
    Returns (table, open set, last result, rounds, truncated selections)."""
    tab = env.alloc_table(1 << 15)
    opn = env.alloc_open(tab)
    sel, imp = patterned_frontier(m, env, cap, 32), m.TableFrontier(env, 1 << 13)
    lists = env.alloc_lists(cap, want_state=True)
    count = tab.seed(start, frontier=imp)
    want_imp, _ = table.seed(start, [h0])
    assert_frontier_equal(imp.download(count), want_imp, "seed")
    opn.push(imp, n_max=count, eps=eps, sight=sight)
    model.push(want_imp, count, eps, sight)
    rounds = truncated = 0
    while True:
        what = "round %d" % rounds
        assert_open_equal(opn, model, what)
        got, want_sel = select_both(opn, model, delta, sel, what)
        n = got["count"]
        if got["status"] != OM.SELECTED or rounds >= max_rounds:
            break
        truncated += n == cap and any(fl & OM.IS_OPEN and model.f[i] <= got["f_min"] + delta for i, fl in model.flags.items())
        env.expand_lists_resident(sel, lists, n_nodes=n)
        cnt = tab.relax(lists, sel.id, sel.g, g_max, frontier=imp, n_nodes=n)
        want_imp, _ = table.relax(lists.download_nodes(0, n), want_sel["id"], want_sel["g"], g_max)
        assert_frontier_equal(imp.download(cnt), want_imp, what + ": relax")
        opn.push(imp, n_max=n * lists.stride, eps=eps, sight=sight)
        model.push(want_imp, n * lists.stride, eps, sight)
        rounds += 1
    assert_spare_untouched(sel)
    for b in (sel, imp, lists):
        b.free()
    return tab, opn, got, rounds, truncated


def small_world_goal(m, O, dim, control, g_max, edge):
    """(workload, start, its hash, goal row): the goal is the position of the farthest node (largest g, smallest id) of a
    model sweep bounded by g_max."""
    wl = _small_world(m, dim, control, seed=5, edge=edge)
    start = small_start(wl)
    if control & 0x08:  # the SNP worlds start with live acc and jerk rows
        start = np.array(CM.live_start(start, dim, control))
    h0 = O.lattice_hash(dim, control, start)
    t = TableModel(4 * dim + 2)
    sweep(t, oracle_provider(O, oracle_env(wl)), start, [h0], g_max=g_max)
    a = t.arrays()
    goal = np.zeros(4 * dim + 2)
    goal[:dim] = a["state"][:dim, int(np.argmax(a["g"]))]
    return wl, start, h0, goal


# (dim, control, g_max, edge) -> per (eps, delta, capacity): rounds, truncated selections (the model's, on the oracle's
# lists: the rounds of the issue's prototype)
WORLDS = {(2, 0x03, 56.0, 32): {(1.0, 0.0, 8192): (95, 0), (1.0, 5.0, 16): (16, 13), (3.0, 5.0, 8192): (4, 0)},
          (3, 0x07, 46.0, 64): {(1.0, 0.0, 8192): (45, 0), (1.0, 5.0, 16): (15, 13), (3.0, 5.0, 8192): (4, 0)}}
OLD_WORLDS = sorted(WORLDS)
WORLDS[CM.SNP_WORLD] = CM.SNP_WORLD_ROUNDS  # 2D SNP from live acc and jerk rows (tests/control_matrix.py)
_goals = {}


def model_search_on_oracle(O, wl, dim, control, start, h0, goal, eps, delta, cap, g_max, w, v_max, max_rounds=10 ** 6):
    """The loop of device_search on the models alone, fed with the oracle's lists (no GPU).  Returns (status, rounds,
    truncated selections, closed nodes at the end, re-opened nodes, nodes)."""
    provider = oracle_provider(O, oracle_env(wl))
    table = TableModel(4 * dim + 2)
    model = OM.OpenModel(table, dim, goal, O.lattice_hash(dim, control, goal), w, v_max, tol_pos=wl.res,
                         blocked=OM.ray_blocked(wl.grid, wl.map_dim, wl.origin, wl.res, goal[:dim]))
    imp, _ = table.seed(start, [h0])
    model.push(imp, imp["count"], eps, True)
    rounds = truncated = reopened = 0
    while True:
        got, sel = model.select(delta, cap)
        n = got["count"]
        if got["status"] != OM.SELECTED or rounds >= max_rounds:
            break
        truncated += n == cap and any(fl & OM.IS_OPEN and model.f[i] <= got["f_min"] + delta for i, fl in model.flags.items())
        lists = provider(sel["state"])
        imp, _ = table.relax(lists, sel["id"], sel["g"], g_max)
        reopened += sum(1 for i in imp["id"] if int(i) in model.flags and not model.flags[int(i)] & OM.IS_OPEN)
        model.push(imp, n * int(lists["stride"]), eps, True)
        rounds += 1
    closed = sum(1 for fl in model.flags.values() if fl & OM.SEEN and not fl & OM.IS_OPEN)
    return got["status"], rounds, truncated, closed, reopened, table.n_nodes


@pytest.mark.parametrize("case", [(1.0, 0.0, 8192), (1.0, 5.0, 16), (3.0, 5.0, 8192)])
@pytest.mark.parametrize("world", OLD_WORLDS + [pytest.param(CM.SNP_WORLD, id="2d-snp")])
def test_search_round_by_round(engine, oracle_lib, world, case):
    """2D ACC, 3D JRK and 2D SNP to FOUND, with the ray trace, every round compared; the rounds are the model's on the
    oracle."""
    m, O = engine, oracle_lib
    dim, control, g_max, edge = world
    eps, delta, cap = case
    if world not in _goals:
        _goals[world] = small_world_goal(m, O, dim, control, g_max, edge)
    wl, start, h0, goal = _goals[world]
    env = engine_env(m, wl)
    env.set_goal(goal, tol_pos=wl.res)
    table = TableModel(4 * dim + 2)
    model = OM.OpenModel(table, dim, goal, O.lattice_hash(dim, control, goal), env._p.w, env._p.v_max, tol_pos=wl.res,
                         blocked=OM.ray_blocked(wl.grid, wl.map_dim, wl.origin, wl.res, goal[:dim]))
    if world not in OLD_WORLDS:  # the pinned numbers are the model's on the oracle: held before the device runs
        status, n_rounds, n_trunc, closed, reopened, nodes = model_search_on_oracle(
            O, wl, dim, control, start, h0, goal, eps, delta, cap, g_max, env._p.w, env._p.v_max)
        print("model on the oracle:", world, case, status, n_rounds, n_trunc, "closed", closed, "re-opened", reopened, "nodes", nodes)
        assert status == OM.FOUND and (n_rounds, n_trunc) == WORLDS[world][case] and n_rounds >= 3
        assert closed + reopened >= 1 and 100 <= nodes <= 20000
    tab, opn, got, rounds, truncated = device_search(m, env, table, model, start, h0, eps, delta, cap, g_max, True, 10 ** 6)
    print(world, case, rounds, truncated, got)
    assert got["status"] == OM.FOUND and (rounds, truncated) == WORLDS[world][case]
    assert_table_equal(tab, table)
    ids, act = tab.path(got["goal_id"])
    assert ids[0] == 0 and ids[-1] == got["goal_id"] and len(act) >= 3
    opn.free()
    tab.free()
    env.close()


def four_rounds_with_yaw(m, O, control, live=False):
    wl = _small_world(m, 2, control, seed=5, edge=32)
    start = small_start(wl)
    if live:
        start = np.array(CM.live_start(start, 2, control))
    goal = np.zeros(10)
    goal[:2] = start[:2] + [1.2, -0.8]
    env = engine_env(m, wl)
    env.set_goal(goal, tol_pos=wl.res)
    table = TableModel(10)
    model = OM.OpenModel(table, 2, goal, O.lattice_hash(2, control, goal), env._p.w, env._p.v_max, tol_pos=wl.res,
                         blocked=OM.ray_blocked(wl.grid, wl.map_dim, wl.origin, wl.res, goal[:2]))
    tab, opn, got, rounds, _ = device_search(m, env, table, model, start, O.lattice_hash(2, control, start), 1.0, 2.0, 8192,
                                             math.inf, True, 4)
    assert rounds == 4 and table.n_nodes > 30 and got["status"] == OM.SELECTED
    assert_table_equal(tab, table)
    opn.free()
    tab.free()
    env.close()


def test_four_rounds_with_yaw_controls(engine, oracle_lib):
    four_rounds_with_yaw(engine, oracle_lib, 0x13)


def test_four_rounds_with_jrk_yaw_controls(engine, oracle_lib):
    """The JRKxYAW twin, from a live acc row: the seed's hash folds it and K = 3 with a heading limit runs the relax and
    the push."""
    four_rounds_with_yaw(engine, oracle_lib, 0x17, live=True)


def corridor_env(m, cells=None):
    c = corridor()
    env = m.EnvMap(2)
    env.setMap(c["origin"], c["dim"], c["cells"] if cells is None else cells, c["res"])
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    start = m.Waypoint(2, m.ACC, pos=c["start"]).to_row()
    goal = m.Waypoint(2, m.ACC, pos=c["goal"]).to_row()
    return env, start, goal


def test_corridor_search_and_path(engine):
    """EnvMap.search with its defaults (eps 1, delta = w dt = 10, the ray trace) on the corridor of test_planner_2d: the
    published cost, the model's expansions and nodes, and the path as a rollout: the same cost and end state, bit for bit."""
    m = engine
    env, start, goal = corridor_env(m)
    table, _, want = corridor_search(m, 1.0, 10.0, 4096, sight=1)
    res = env.search(start, goal, capacity=1 << 15, max_frontier=4096)
    print(res, res.last_select, want)
    assert res.status == m.search.FOUND and res.found and res.cost == 351.5
    assert (res.rounds, res.expanded) == (want["rounds"], want["expanded"])
    assert_result_equal(res.last_select, want["result"])
    got = assert_table_equal(res.table, table)
    assert res.expanded < got["n_nodes"] < 21677  # (the bounded sweep's nodes, without a bound known in advance)
    start_state, act = res.path()
    assert len(act) == 35 and np.array_equal(bits(start_state), bits(start))
    r = env.rollout(start_state, act.reshape(-1, 1), want_goal_rows=True)
    assert r["status"][0] == m.SLOT_FINITE and r["steps"][0] == 35
    assert bits(r["cost"])[0] == bits([res.cost])[0]
    # the end state is the goal node: its lattice hash, and bit for bit every row the hash of an ACC state covers (pos,
    # vel), yaw and t.  The acc row is the last control input: the table keeps the state of the edge that CREATED the
    # node (mplx_table.h: never rewritten), the rollout has that of the best edge -- here -0.5 and 0.
    assert r["end_hash"][0] == got["hash"][res.goal_id]
    rows = [0, 1, 2, 3, 8, 9]
    assert np.array_equal(bits(r["end_state"][rows, 0]), bits(got["state"][rows, res.goal_id]))
    assert r["end_flags"][0] & 1 and bits([res.cost + 1.0 * r["end_heur"][0]])[0] == bits([res.last_select["goal_f"]])[0]
    res.free()
    env.close()


def test_empty_and_the_limits(engine):
    m = engine
    cells = blocked_goal_cells()
    env, start, goal = corridor_env(m, cells)
    _, table, opn, prov, s0, h0 = corridor_setup(m, cells=cells)
    want = OM.search(table, opn, prov, s0, h0, 1.0, 10.0, 4096, g_max=60.0)
    res = env.search(start, goal, g_max=60.0, capacity=1 << 15, max_frontier=4096, sight=False)
    assert res.status == m.search.EMPTY == want["status"] and not res.found and res.cost == math.inf and res.goal_id == -1
    assert (res.rounds, res.expanded) == (want["rounds"], want["expanded"]) and res.expanded > 50
    assert_result_equal(res.last_select, want["result"])
    with pytest.raises(RuntimeError):
        res.path()
    res.free()
    env.close()
    env, start, goal = corridor_env(m)
    for kw, status in (({"max_rounds": 5}, m.search.MAX_ROUNDS), ({"max_expand": 40}, m.search.MAX_EXPAND)):
        _, opn, want = corridor_search(m, 1.0, 10.0, 4096, sight=1, **kw)
        res = env.search(start, goal, capacity=1 << 15, max_frontier=4096, **kw)
        assert res.status == status == want["status"] and not res.found and res.cost == math.inf
        assert (res.rounds, res.expanded) == (want["rounds"], want["expanded"])
        assert_open_equal(res.open, opn, str(kw))  # the selection is open again
        res.free()
    with pytest.raises(RuntimeError, match="table status"):
        env.search(start, goal, capacity=256)
    env.close()


def test_argument_errors_and_state(engine):
    m = engine
    L_ = m._abi.lib()
    ARG, STATE = m._abi.ERR_ARG, m._abi.ERR_STATE
    env = rest_env(m)
    tab = env.alloc_table(64)
    o = C.c_void_p()
    assert L_.mplx_open_create(None, C.byref(o)) == ARG and L_.mplx_open_create(tab._tab, None) == ARG
    opn = env.alloc_open(tab)
    fr = m.TableFrontier(env, 8)
    fr.count.upload(np.array([0], np.int64))
    inf, nan = float("inf"), float("nan")
    res = m._abi.OpenResult()

    def push(f=None, n_max=1, eps=1.0, sight=0, o=opn._open):
        f = fr.c_struct() if f is None else f
        return L_.mplx_open_push_device(o, C.byref(f), n_max, eps, sight)

    def select(f=None, delta=0.0, o=opn._open):
        f = fr.c_struct() if f is None else f
        return L_.mplx_open_select_device(o, delta, C.byref(f), None, C.byref(res))
    # no goal yet
    assert push() == STATE
    goal = np.zeros(10)
    env.set_goal(goal)
    assert push() == m._abi.OK
    assert push(sight=1) == STATE  # no map
    assert push(o=None) == ARG and select(o=None) == ARG
    assert L_.mplx_open_push_device(opn._open, None, 1, 1.0, 0) == ARG
    assert L_.mplx_open_select_device(opn._open, 0.0, None, None, None) == ARG
    assert push(n_max=-1) == ARG
    for eps in (nan, -1.0, inf):
        assert push(eps=eps) == ARG, eps
    for delta in (nan, -0.5, -inf):
        assert select(delta=delta) == ARG, delta
    for field, v in (("id", None), ("g", None), ("state", None), ("count", None), ("state_stride", 7), ("capacity", -1)):
        f = fr.c_struct()
        setattr(f, field, v)
        assert push(f=f) == ARG and select(f=f) == ARG, field
    assert L_.mplx_open_view_of(opn._open, None) == ARG and L_.mplx_open_clear(None) == ARG
    # nothing of the above touched anything
    assert select(delta=inf) == m._abi.OK and res.status == OM.EMPTY and res.count == 0
    # a table with a status bit: 40 new keys into 8 free nodes
    from test_gpu_table import distinct_list, upload, upload_lists
    lists = upload_lists(m, env, distinct_list(np.random.default_rng(3), 40))
    pid, pg = upload(env, m, np.zeros(1, np.int32)), upload(env, m, np.zeros(1))
    small = env.alloc_table(8)
    sopn = env.alloc_open(small)
    big = m.TableFrontier(env, 64)
    small.relax(lists, pid, pg, frontier=big, want_count=False)
    sopn.push(big, n_max=40, eps=1.0)  # queued before the host has seen the bit: does nothing
    with pytest.raises(m._abi.MplxError) as err:
        sopn.select(0.0, big)
    assert err.value.code == STATE and small.stats()[1] & m.table.NODES_FULL
    for call in (lambda: sopn.push(big, n_max=1), lambda: sopn.select(0.0, big), sopn.clear, lambda: env.alloc_open(small)):
        with pytest.raises(m._abi.MplxError) as err:
            call()
        assert err.value.code == STATE
    small.clear()
    sopn.clear()
    assert sopn.select(0.0, big)["status"] == OM.EMPTY
    for b in (fr, lists, pid, pg, big):
        b.free()
    sopn.free()
    small.free()
    opn.free()
    tab.free()
    env.close()
