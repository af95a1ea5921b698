"""GPU: the node table of include/mplx_table.h against tests/table_model.py run on the SAME lists (hand-built, or
downloaded from the device, so that yaw controls are exact too).  Every comparison is exact -- relax only adds and
compares doubles: node arrays, n_nodes, entry ids and the frontier (ids, g, state rows, order, count) bit for bit."""
import ctypes as C
import math

import numpy as np
import pytest

import control_matrix as CM
import prior_model
from helpers import engine_env, oracle_env
from table_model import EMPTY, F2, TableModel, dijkstra, hand_case, hand_lists, oracle_provider, sweep
from test_gpu_parity import _small_world
from test_plan_known_answer import corridor
from test_table import small_start

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def upload_lists(m, env, host):
    """env.Lists holding the host lists (mplx_succ_lists layout, "stride" S)."""
    n, S = len(host["count"]), int(host["stride"])
    L = m.Lists(env, n, S, want_state=True, stride=S)
    L.count.upload(host["count"].astype(np.int32))
    L.action.upload(host["action"].astype(np.int32))
    L.cost.upload(host["cost"].astype(np.float64))
    L.hash.upload(host["hash"].astype(np.uint64))
    st = np.zeros((L.n_fields, L.state_stride))
    st[:, :n * S] = host["state"]
    L.state.upload(st)
    L.zero_rows = 0
    return L


def upload(env, m, a):
    buf = m.DeviceArray(env, max(a.nbytes, 8))
    buf.upload(a)
    return buf


def relax_both(m, env, tab, model, host, parent_id, parent_g, g_max, fcap=None, spare=0):
    """One relax call on the device and in the model; returns (device frontier, device entry ids, model frontier, model
    entry ids, count the call reported)."""
    n, S = len(host["count"]), int(host["stride"])
    L = upload_lists(m, env, host)
    d_pid, d_pg = upload(env, m, parent_id.astype(np.int32)), upload(env, m, parent_g.astype(np.float64))
    d_eid = upload(env, m, np.full(n * S, -7, np.int32))
    fr = m.TableFrontier(env, n * S if fcap is None else fcap, spare)
    cnt = tab.relax(L, d_pid, d_pg, g_max, frontier=fr, entry_id=d_eid)
    got_fr, got_eid = fr.download(cnt), d_eid.download(np.int32, (n * S,))
    want_fr, want_eid = model.relax(host, parent_id, parent_g, g_max)
    for b in (d_pid, d_pg, d_eid, fr, L):
        b.free()
    return got_fr, got_eid, want_fr, want_eid, cnt


def assert_frontier_equal(got, want, what=""):
    assert got["count"] == want["count"], what
    assert np.array_equal(got["id"], want["id"]), what + ": frontier ids / order"
    assert np.array_equal(bits(got["g"]), bits(want["g"])), what + ": frontier g"
    assert np.array_equal(bits(got["state"]), bits(want["state"])), what + ": frontier state rows"


def assert_table_equal(tab, model, what=""):
    got, want = tab.download(), model.arrays()
    assert got["status"] == 0, what
    assert got["n_nodes"] == want["n_nodes"], what
    assert np.array_equal(got["hash"], want["hash"]), what + ": hash / creation order"
    assert np.array_equal(bits(got["g"]), bits(want["g"])), what + ": g"
    assert np.array_equal(got["pred"], want["pred"]), what + ": pred"
    assert np.array_equal(got["pred_action"], want["pred_action"]), what + ": pred_action"
    assert np.array_equal(bits(got["state"]), bits(want["state"])), what + ": state"
    return got


def bare_env(m):
    """A 2D context without map or controls: relax needs neither."""
    return m.EnvMap(2)


def test_one_relax_on_hand_built_lists(engine):
    """300 nodes x 40 entries: three scan tiles, a stride that is no multiple of 32, shared hashes, ties, +inf / NaN
    costs, a parent without id, poisoned tails, the empty-marker hash and a g_max that cuts."""
    m = engine
    rng, pool, host, parent_id, parent_g = hand_case()
    env = bare_env(m)
    tab, model = env.alloc_table(4096), TableModel(F2)
    got_fr, got_eid, want_fr, want_eid, cnt = relax_both(m, env, tab, model, host, parent_id, parent_g, g_max=3.25)
    assert cnt == want_fr["count"] and 500 < cnt < model.n_nodes + 1
    assert np.array_equal(got_eid, want_eid)
    assert (want_eid >= 0).sum() > 3000 and (want_eid < 0).sum() > 3000  # both kinds are there
    assert_frontier_equal(got_fr, want_fr)
    got = assert_table_equal(tab, model)
    assert EMPTY in got["hash"] and -1 not in got["pred"][got["g"] < np.inf]
    cut = host["cost"] + np.repeat(parent_g, 40)
    assert (cut[np.isfinite(cut)] > 3.25).sum() > 100  # g_max did cut
    # find: every node by its hash; the poisoned hashes and a stranger are not there
    assert np.array_equal(tab.find(got["hash"]), np.arange(got["n_nodes"], dtype=np.int32))
    live = (np.arange(40)[None, :] < host["count"][:, None]).ravel()
    assert np.all(tab.find(host["hash"][~live][:500]) == -1) and tab.find([12345])[0] == -1
    tab.free()
    env.close()


def test_three_calls_on_one_table(engine):
    """Later calls meet existing keys with equal, larger and smaller candidates: equal neither improves nor emits."""
    m = engine
    rng, pool, host, parent_id, parent_g = hand_case(seed=12, n=120, S=40)
    env = bare_env(m)
    tab, model = env.alloc_table(4096), TableModel(F2)
    other = lambda pid, by: np.where(pid < 0, -1, pid + by).astype(np.int32)  # other parents; the one without id stays so
    g1, e1, w1, we1, _ = relax_both(m, env, tab, model, host, parent_id, parent_g, math.inf)
    assert_frontier_equal(g1, w1, "call 1")
    before = assert_table_equal(tab, model, "call 1")
    # the same lists again: every candidate equals or exceeds what the table holds
    g2, e2, w2, we2, cnt2 = relax_both(m, env, tab, model, host, other(parent_id, 5000), parent_g, math.inf)
    assert cnt2 == 0 and w2["count"] == 0 and np.array_equal(e2, we2) and np.array_equal(e2, e1)
    after = assert_table_equal(tab, model, "call 2")
    assert np.array_equal(after["pred"], before["pred"])  # the other parents did not take over on a tie
    # other lists over the same pool, parents cheaper for some and dearer for others, and new keys among them
    host3 = hand_lists(rng, 120, 40, np.concatenate([pool, rng.integers(1, 2 ** 63, size=300, dtype=np.uint64)]), 0xBEEF00000000)
    pg3 = np.maximum(parent_g + rng.choice([-0.5, 0.0, 0.75], size=120), 0.0)
    g3, e3, w3, we3, cnt3 = relax_both(m, env, tab, model, host3, other(parent_id, 9000), pg3, 4.0)
    assert np.array_equal(e3, we3)
    assert_frontier_equal(g3, w3, "call 3")
    final = assert_table_equal(tab, model, "call 3")
    old = before["n_nodes"]
    assert final["n_nodes"] > old and 0 < (final["g"][:old] < before["g"]).sum() < old  # some improved, some not
    assert np.array_equal(bits(final["state"][:, :old]), bits(before["state"]))  # a node's state is never rewritten
    tab.free()
    env.close()


def test_a_nearly_full_hash_table(engine):
    """60 keys in 64 slots: long probe chains that wrap around the end of the table."""
    m = engine
    rng = np.random.default_rng(13)
    pool = rng.integers(1, 2 ** 63, size=60, dtype=np.uint64)
    host = hand_lists(rng, 8, 40, pool, 0xDEAD00000000, inf_rate=0.0, nan_rate=0.0)
    host["count"][:] = 40
    host["hash"] = pool[rng.integers(0, 60, size=320)]
    host["hash"][:60] = pool  # every key at least once
    host["cost"] = rng.choice([0.5, 1.0, 1.5], size=320)
    host["state"] = rng.standard_normal((F2, 320))
    env = bare_env(m)
    tab, model = env.alloc_table(60, slots_log2=6), TableModel(F2)
    pid, pg = np.arange(8, dtype=np.int32), rng.choice([0.0, 0.5], size=8)
    got_fr, got_eid, want_fr, want_eid, _ = relax_both(m, env, tab, model, host, pid, pg, math.inf)
    assert np.array_equal(got_eid, want_eid)
    assert_frontier_equal(got_fr, want_fr)
    got = assert_table_equal(tab, model)
    assert got["n_nodes"] == 60
    assert np.array_equal(tab.find(pool), np.array([model.ids[int(h)] for h in pool], np.int32))
    assert sorted(tab.find(pool).tolist()) == list(range(60))
    # a second call with lower parents goes through the same chains
    got_fr, got_eid, want_fr, want_eid, _ = relax_both(m, env, tab, model, host, pid + 100, pg * 0.5, math.inf)
    assert np.array_equal(got_eid, want_eid)
    assert_frontier_equal(got_fr, want_fr, "second call")
    assert_table_equal(tab, model, "second call")
    tab.free()
    env.close()


def distinct_list(rng, n_keys, S=40):
    """One node whose n_keys entries carry distinct hashes and finite costs."""
    host = {"stride": S, "count": np.array([n_keys], np.int32), "action": np.arange(S, dtype=np.int32),
            "cost": np.full(S, 1.0), "hash": rng.integers(1, 2 ** 63, size=S, dtype=np.uint64), "state": rng.standard_normal((F2, S))}
    host["cost"][n_keys:] = np.nan
    return host


@pytest.mark.parametrize("case", ["nodes", "frontier"])
def test_full_conditions_set_their_bit_and_write_nothing_outside(engine, case):
    """Capacity 16 under 40 new keys; a frontier of 8 under 20 improvements.  The status bit, the 64 spare entries behind
    every frontier row, MPLX_ERR_STATE for the next call, and clear."""
    m = engine
    rng = np.random.default_rng(14)
    env = bare_env(m)
    cap, fcap, n_keys, bit = (16, 64, 40, m.table.NODES_FULL) if case == "nodes" else (64, 8, 20, m.table.FRONTIER_FULL)
    tab = env.alloc_table(cap)
    host = distinct_list(rng, n_keys)
    L = upload_lists(m, env, host)
    pid, pg = upload(env, m, np.zeros(1, np.int32)), upload(env, m, np.zeros(1))
    fr = m.TableFrontier(env, fcap, spare=64)
    pat_i = np.full(fr.state_stride, 0x5A5A5A5A, np.int32)
    pat_d = np.full(fr.state_stride, -1234.5)
    fr.id.upload(pat_i)
    fr.g.upload(pat_d)
    fr.state.upload(np.tile(pat_d, (F2, 1)))
    cnt = tab.relax(L, pid, pg, frontier=fr)
    n_nodes, status = tab.stats()
    assert status & bit and n_nodes <= cap and 0 <= cnt <= fcap
    assert np.array_equal(fr.id.download(np.int32, (fr.state_stride,))[fcap:], pat_i[fcap:])
    assert np.array_equal(bits(fr.g.download(np.float64, (fr.state_stride,))[fcap:]), bits(pat_d[fcap:]))
    st = fr.state.download(np.float64, (F2, fr.state_stride))
    assert np.array_equal(bits(st[:, fcap:]), bits(np.tile(pat_d[fcap:], (F2, 1))))
    with pytest.raises(m._abi.MplxError) as err:
        tab.relax(L, pid, pg, frontier=fr)
    assert err.value.code == m._abi.ERR_STATE
    with pytest.raises(m._abi.MplxError) as err:
        tab.find([1])
    assert err.value.code == m._abi.ERR_STATE
    # clear makes it usable again: a call that fits, against a fresh model
    tab.clear()
    small = distinct_list(rng, 6)
    model = TableModel(F2)
    got_fr, got_eid, want_fr, want_eid, _ = relax_both(m, env, tab, model, small, np.zeros(1, np.int32), np.zeros(1), math.inf, fcap=8)
    assert np.array_equal(got_eid, want_eid)
    assert_frontier_equal(got_fr, want_fr)
    assert_table_equal(tab, model)
    for b in (L, pid, pg, fr):
        b.free()
    tab.free()
    env.close()


def device_sweep(m, env, model, start, h0, g_max, max_rounds, capacity, fcap):
    """The sweep of EnvMap.cost_to_come spelled out, every round compared with the model fed with the device's own
    lists.  Returns (table, rounds, hashes of the seeds as the device computed them)."""
    tab = env.alloc_table(capacity)
    cur, nxt = m.TableFrontier(env, fcap), m.TableFrontier(env, fcap)
    lists = env.alloc_lists(fcap, want_state=True)
    eid = m.DeviceArray(env, lists.n_slots * 4)
    count = tab.seed(start, frontier=cur)
    want, _ = model.seed(start, [h0])
    assert_frontier_equal(cur.download(count), want, "seed")
    rounds = 0
    while count > 0 and rounds < max_rounds:
        env.expand_lists_resident(cur, lists, n_nodes=count)
        new_count = tab.relax(lists, cur.id, cur.g, g_max, frontier=nxt, n_nodes=count, entry_id=eid)
        host = lists.download_nodes(0, count)
        want_next, want_eid = model.relax(host, want["id"], want["g"], g_max)
        rounds += 1
        assert np.array_equal(eid.download(np.int32, (count * lists.stride,)), want_eid), "round %d: entry ids" % rounds
        assert_frontier_equal(nxt.download(new_count), want_next, "round %d" % rounds)
        cur, nxt, want, count = nxt, cur, want_next, new_count
    for b in (cur, nxt, lists, eid):
        b.free()
    return tab, rounds


@pytest.mark.parametrize("dim,control,g_max,max_rounds,edge", [(2, 0x03, 56.0, 99, 32), (3, 0x07, 46.0, 99, 64), (2, 0x13, math.inf, 4, 32)] +
                         [pytest.param(*c[1:], id=c[0]) for c in CM.SWEEP_ADDED])
def test_sweeps_round_by_round(engine, oracle_lib, dim, control, g_max, max_rounds, edge):
    """2D ACC (six rounds, six candidates per node) and 3D JRK (five rounds; a 3.2 m map ends every third step outside)
    to the fixed point inside g_max, and four rounds of 2D ACC x YAW.  The cases of tests/control_matrix.py: 2D and 3D SNP
    to the fixed point, four rounds of 2D JRK x YAW, 3D VEL x YAW and 2D SNP x YAW, all from a start whose acc and jerk rows
    are live where the order has them."""
    m, O = engine, oracle_lib
    wl = _small_world(m, dim, control, seed=5, edge=edge)
    start = small_start(wl)
    added = [c for c in CM.SWEEP_ADDED if c[1:] == (dim, control, g_max, max_rounds, edge)]
    if added:
        start = np.array(CM.live_start(start, dim, control))
        # the choice of g_max and the map edge, on the model fed with the oracle's lists, before the device runs
        probe = TableModel(4 * dim + 2)
        n_rounds, _ = sweep(probe, oracle_provider(O, oracle_env(wl)), start, [O.lattice_hash(dim, control, start)], g_max=g_max,
                            max_rounds=max_rounds)
        print("model on the oracle:", added[0][0], "rounds", n_rounds, "nodes", probe.n_nodes)
        assert n_rounds >= 3 and 100 < probe.n_nodes <= 20000
        if CM.SWEEP_MODEL[added[0][0]] is not None:
            assert (n_rounds, probe.n_nodes) == CM.SWEEP_MODEL[added[0][0]]
    env = engine_env(m, wl)
    h0 = O.lattice_hash(dim, control, start)
    model = TableModel(4 * dim + 2)
    tab, rounds = device_sweep(m, env, model, start, h0, g_max, max_rounds, capacity=1 << 15, fcap=1 << 13)
    got = assert_table_equal(tab, model)
    assert got["n_nodes"] > 100 and rounds >= 3, (got["n_nodes"], rounds)
    if not control & 0x10:
        want = dijkstra(oracle_provider(O, oracle_env(wl)), start, h0, g_max)
        assert {int(h): float(g) for h, g in zip(got["hash"], got["g"])} == want
    # every chain of best predecessors ends at the seed and its actions are the nodes' own
    last = got["n_nodes"] - 1
    ids, act = tab.path(last)
    assert ids[0] == 0 and ids[-1] == last and np.array_equal(ids[:-1], got["pred"][ids[1:]])
    assert np.array_equal(act, got["pred_action"][ids[1:]])
    with pytest.raises(m._abi.MplxError) as err:
        tab.path(last, cap=len(act) - 1)
    assert err.value.code == m._abi.ERR_ARG
    tab.free()
    env.close()


def hash_states(dim, control, n=70):
    """n states whose every row the hash of `control` folds is live: values across many bins, on the bins' edges (halves
    round away from zero), negative and signed zeros."""
    rng = np.random.default_rng(31 * dim + control)
    s = np.zeros((4 * dim + 2, n))
    s[:dim] = np.round(rng.uniform(-3.0, 9.0, size=(dim, n)), 3)
    s[dim:4 * dim] = np.round(rng.uniform(-2.0, 2.0, size=(3 * dim, n)), 2)
    s[4 * dim] = np.round(rng.uniform(-3.1, 3.1, size=n), 2)
    s[:dim, 1], s[dim:4 * dim, 1], s[4 * dim, 1] = 0.005, 0.05, 0.05     # every row on a bin edge
    s[:dim, 2], s[dim:4 * dim, 2], s[4 * dim, 2] = -0.015, -0.25, -0.15
    s[:4 * dim + 1, 3] = -0.0
    s[3 * dim:4 * dim, 4:10] = 0.1 * np.arange(1, 7)                      # one jerk bin apart, everything else as in column 4
    s[:3 * dim, 5:10] = s[:3 * dim, 4:5]
    s[4 * dim, 5:10] = s[4 * dim, 4]
    s[4 * dim + 1] = np.arange(n) * 0.5
    return s


@pytest.mark.parametrize("dim,control", CM.PAIRS, ids=["%dd-%s" % (d, c.lower()) for d, c in CM.PAIRS])
def test_seed_hashes_equal_the_oracle(engine, oracle_lib, dim, control):
    """table_hash_kernel<D, K, YAW> for all 16 (dim, control): the hash column of seeded states against the oracle's
    lattice hash and the restatement of tests/prior_model.py, state by state."""
    m, O = engine, oracle_lib
    flag = CM.FLAGS[control]
    env = m.EnvMap(dim)
    env.setMap([0.0] * dim, [8] * dim, np.zeros(8 ** dim, np.int8), 1.0)
    env.set_control(flag)
    env.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], dim, yaw_rates=[-0.3, 0.0, 0.3]) if flag & 0x10 else
              m.workloads.grid_controls([-0.5, 0.0, 0.5], dim))
    env.set_dt(1.0)
    states = hash_states(dim, flag)
    n = states.shape[1]
    want = np.array([O.lattice_hash(dim, flag, states[:, k]) for k in range(n)], dtype=np.uint64)
    assert want.tolist() == [prior_model.lattice_hash(dim, flag, states[:, k]) for k in range(n)]
    first = {}
    for k, h in enumerate(want.tolist()):
        first.setdefault(h, k)
    # the jerk row decides at order 4 and only there: six states one jerk bin apart
    assert len(set(want[4:10].tolist())) == (6 if CM.order_of(flag) == 4 else 1)
    tab = env.alloc_table(256)
    fr = m.TableFrontier(env, n)
    assert tab.seed(states, frontier=fr) == len(first)  # a state whose hash an earlier one has is that node
    got = tab.download()
    assert got["n_nodes"] == len(first) and np.array_equal(got["hash"], want[sorted(first.values())])
    assert np.array_equal(bits(got["state"]), bits(states[:, sorted(first.values())]))
    fr.free()
    tab.free()
    env.close()


def test_corridor_sweep_and_path(engine):
    """The corridor of test_planner_2d through EnvMap.cost_to_come: the rounds and nodes of the CPU test, the published
    cost at the goal, and its path as a rollout: the same cost and the same end state, bit for bit."""
    m = engine
    c = corridor()
    env = m.EnvMap(2)
    env.setMap(c["origin"], c["dim"], c["cells"], c["res"])
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    env.set_v_max(1.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    start = m.Waypoint(2, m.ACC, pos=c["start"]).to_row()
    tab, rounds = env.cost_to_come(start, g_max=351.5, capacity=1 << 15, max_frontier=2048)
    got = tab.download()
    assert rounds == 36 and got["n_nodes"] == 21677 and got["status"] == 0
    near = np.nonzero(np.abs(got["state"][:2] - np.asarray(c["goal"])[:, None]).max(axis=0) <= 0.5)[0]
    assert near.size == 1 and got["g"][near[0]] == 351.5
    ids, act = tab.path(int(near[0]))
    assert len(act) == 35 and ids[0] == 0
    assert np.array_equal(bits(tab.state_of(0)), bits(start))
    r = env.rollout(tab.state_of(ids[0]), act.reshape(-1, 1))
    assert r["status"][0] == m.SLOT_FINITE and r["steps"][0] == 35
    assert bits(r["cost"])[0] == bits(got["g"][near[0]:near[0] + 1])[0]
    assert np.array_equal(bits(r["end_state"][:, 0]), bits(got["state"][:, near[0]]))
    tab.free()
    env.close()


def test_argument_errors(engine):
    m = engine
    L_ = m._abi.lib()
    env = bare_env(m)
    t = C.c_void_p()
    for cap, log2 in ((0, 0), (1 << 31, 0), (64, 6), (64, 5), (8, 32)):
        assert L_.mplx_table_create(env._ctx, cap, log2, C.byref(t)) == m._abi.ERR_ARG, (cap, log2)
    assert L_.mplx_table_create(env._ctx, 8, 0, None) == m._abi.ERR_ARG
    tab = env.alloc_table(64)
    fr = m.TableFrontier(env, 8)
    host = distinct_list(np.random.default_rng(1), 4)
    lists = upload_lists(m, env, host)
    pid, pg = upload(env, m, np.zeros(1, np.int32)), upload(env, m, np.zeros(1))
    inf = float("inf")

    def relax(s, n=1, f=None, p=pid.ptr, g=pg.ptr):
        f = fr.c_struct() if f is None else f
        return L_.mplx_table_relax_device(tab._tab, C.byref(s) if s is not None else None, n, p, g, inf, C.byref(f), None, None)
    assert relax(None) == m._abi.ERR_ARG
    assert relax(lists.c_struct(), n=-1) == m._abi.ERR_ARG
    assert relax(lists.c_struct(), p=None) == m._abi.ERR_ARG and relax(lists.c_struct(), g=None) == m._abi.ERR_ARG
    for row in ("count", "action", "cost", "hash", "state"):
        s = lists.c_struct()
        setattr(s, row, None)
        assert relax(s) == m._abi.ERR_ARG, row
    s = lists.c_struct()
    s.state_stride = 39
    assert relax(s) == m._abi.ERR_ARG
    for field, v in (("id", None), ("g", None), ("state", None), ("count", None), ("state_stride", 7), ("capacity", -1)):
        f = fr.c_struct()
        setattr(f, field, v)
        assert relax(lists.c_struct(), f=f) == m._abi.ERR_ARG, field
    # a seed needs parameters and controls; this context has neither
    st = np.zeros((F2, 1))
    f = fr.c_struct()
    assert L_.mplx_table_seed(tab._tab, st.ctypes.data, 1, 1, None, C.byref(f), None) == m._abi.ERR_STATE
    assert L_.mplx_table_seed(tab._tab, st.ctypes.data, 2, 1, None, C.byref(f), None) == m._abi.ERR_ARG
    n = C.c_int64()
    ids = np.zeros(4, np.int32)
    assert L_.mplx_table_path(tab._tab, 0, None, ids.ctypes.data, 3, C.byref(n)) == m._abi.ERR_ARG
    assert L_.mplx_table_path(tab._tab, 0, ids.ctypes.data, ids.ctypes.data, 3, C.byref(n)) == m._abi.ERR_ARG  # an empty table
    assert L_.mplx_table_find(tab._tab, None, 3, ids.ctypes.data) == m._abi.ERR_ARG
    # nothing of the above touched the table; zero nodes are a no-op with an empty frontier
    fr.count.upload(np.array([99], np.int64))
    assert tab.relax(lists, pid, pg, frontier=fr, n_nodes=0) == 0 and fr.count.download(np.int64, (1,))[0] == 0
    assert tab.stats() == (0, 0)
    assert tab.relax(lists, pid, pg, frontier=fr) == 4 and tab.stats() == (4, 0)
    for b in (lists, pid, pg, fr):
        b.free()
    tab.free()
    env.close()
