"""mplx_shortcut on the device (include/mplx_limits.h, csrc/limits_kernel.hip) against tests/shortcut_model.py.

ACC in 2-D is bit for bit: the edge costs are the model's, computed from the pair coefficients the device returned (the
efforts and traversals are exact given the coefficients, and the limits of a cubic never leave the IEEE-only branches),
and keep / cost / chain_cost are the model's programme on that matrix.  JRK in 3-D on a potential map is held to the
invariants that do not depend on the device library: cost <= chain_cost exactly (rounding is monotone), the ends kept,
every non-adjacent hop taken valid and collision free, the result's segments the chosen pairs' (through every call that
reads them, against a host load of the same segments), a repeated t a BAD_CHAIN for that query only."""
import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import shortcut_model as XM
from test_gpu_solve import same_bits

pytestmark = pytest.mark.gpu

MAP2 = ([40, 40], [0.0, 0.0], 0.25)
W_TIME = 10.0


def detour_chain():
    """9 ACC states in 2-D that climb over x = 5 at y >= 4: pos, vel by central differences, t = 0 .. 8."""
    pos = np.array([[1, 2], [2, 2], [3, 2.5], [4, 4], [5, 5], [6, 4], [7, 2.5], [8, 2], [9, 2]], float)
    vel = np.zeros_like(pos)
    vel[1:-1] = (pos[2:] - pos[:-2]) / 2.0
    st = np.zeros((10, 9, 1))
    st[0:2, :, 0], st[2:4, :, 0], st[9, :, 0] = pos.T, vel.T, np.arange(9.0)
    return st


def env2(m, grid):
    md, org, res = MAP2
    env = m.EnvMap(2)
    env.setMap(org, md, grid.ravel(), res)
    env.set_control(m.ACC)
    env.set_v_max(2.0)
    env.set_a_max(1.5)
    env.set_w(W_TIME)
    return env


def check_against_model(m, env, res, grid, W, hop, control, so, D):
    md, org, rs = MAP2
    world = (grid.ravel(), None, md, org, rs, 2.0, 0.1, 0.0)
    want = XM.edge_costs(res.pairs, hop, D, so, control, W_TIME, (2.0, 1.5, 0.0), world)
    same_bits(res.edge_cost.reshape(-1), want, "edge costs")
    for k in range(len(res.keep)):
        status, keep, cost, chain = XM.dp(res.edge_cost[k], W, hop)
        assert res.status[k] == status and res.keep[k].tolist() == keep, (k, res.keep[k], keep)
        same_bits([res.cost[k], res.chain_cost[k]], [cost, chain], "cost and chain_cost of query %d" % k)


def test_acc_2d_bit_for_bit(engine):
    m = engine
    st = detour_chain()
    grid = np.zeros((40, 40), np.int8)
    env = env2(m, grid)
    env.set_potential_weight(0.1)
    free = env.shortcut(st, control=m.ACC, max_hop=8)
    assert free.status.tolist() == [0] and free.pairs.n == 64 and free.edge_cost.shape == (1, 8, 8)
    check_against_model(m, env, free, grid, 9, 8, m.ACC, 1, 2)
    assert len(free.keep[0]) < 9 and free.cost[0] < free.chain_cost[0]
    assert np.isfinite(free.edge_cost[0, 0, 7])  # the straight hop 0 -> 8 is admitted on the free map
    # a wall two cells thick below the chain's crest: the hops through it are +inf, the chosen chain goes round
    grid[0:16, 19:21] = 100  # x in [4.75, 5.25), y in [0, 4)
    env.setMap(MAP2[1], MAP2[0], grid.ravel(), MAP2[2])
    wall = env.shortcut(st, control=m.ACC, max_hop=8)
    check_against_model(m, env, wall, grid, 9, 8, m.ACC, 1, 2)
    assert np.isinf(wall.edge_cost[0, 0, 7]) and np.isinf(wall.edge_cost[0, 1:4, 3:]).any()
    keep = wall.keep[0].tolist()
    assert keep != free.keep[0].tolist() and any(3 <= i <= 5 for i in keep), keep
    trav = wall.poly.traverse()
    assert wall.status[0] == 0 and np.isfinite(trav["cost"][0]) and wall.poly.n_segs[0] == len(keep) - 1
    same_bits(wall.poly.taus()[:len(keep), 0], np.concatenate([[0.0], np.cumsum(np.diff(np.array(keep, float)))]), "taus")
    one = env.shortcut(st, control=m.ACC, max_hop=1)
    check_against_model(m, env, one, grid, 9, 1, m.ACC, 1, 2)
    assert one.keep[0].tolist() == list(range(9)) and one.cost[0] == one.chain_cost[0] and one.pairs.n == 8
    for r in (free, wall, one):
        r.free()
    env.close()


def test_invariants_jrk_3d_potential(engine):
    m, D, W, Q = engine, 3, 6, 5
    md, org, res = ([24, 21, 19], [-1.0, 0.5, -0.3], 0.25)
    rng = np.random.default_rng(77)
    pot = rng.integers(0, 60, md[0] * md[1] * md[2]).astype(np.int8)
    env = m.EnvMap(D)
    env.setMap(org, md, np.zeros(pot.size, np.int8), res)
    env.set_control(m.JRK)
    env.set_v_max(1.5)
    env.set_a_max(1.2)
    env.set_w(W_TIME)
    env.set_potential_weight(0.1)
    env.set_gradient_weight(0.25)
    env.set_potential_map(pot)
    st = np.zeros((14, W, Q))
    for k in range(Q):
        p = np.array([0.5, 1.5, 0.8]) + rng.uniform(0, 0.5, 3)
        step = rng.uniform(0.2, 0.6, 3)
        for w in range(W):
            st[0:3, w, k] = p + step * w + rng.uniform(-0.1, 0.1, 3) * (0 < w < W - 1)
            st[3:6, w, k] = step / 1.0 + rng.uniform(-0.1, 0.1, 3)
            st[6:9, w, k] = rng.uniform(-0.1, 0.1, 3)
            st[13, w, k] = 1.0 * w
    n_wp = np.array([6, 0, 4, 6, 2], np.int32)
    st[13, 3, 3] = st[13, 2, 3]  # query 3: a repeated t
    r = env.shortcut(st, n_wp=n_wp, control=m.JRK, max_hop=4)
    assert r.status.tolist() == [0, m.SOLVE_EMPTY, 0, m.SHORTCUT_BAD_CHAIN, 0]
    assert r.keep[3].tolist() == list(range(6)) and np.isnan(r.cost[3]) and np.isnan(r.chain_cost[3]) and len(r.keep[1]) == 0
    pl, pt = r.pairs.limits(all_roots=True), r.pairs.traverse()
    seg, dts = r.pairs.segments(), r.pairs.dts()
    coeff, durs, n_segs = np.zeros((W - 1, D + 1, 6, Q)), np.ones((W - 1, Q)), np.zeros(Q, np.int32)
    for k in (0, 2, 4):
        keep = r.keep[k].tolist()
        assert r.cost[k] <= r.chain_cost[k] and keep[0] == 0 and keep[-1] == n_wp[k] - 1 and keep == sorted(set(keep))
        for s, (i, j) in enumerate(zip(keep, keep[1:])):
            p = (k * (W - 1) + i) * 4 + (j - i - 1)
            assert j - i <= 4 and r.pairs.status[p] == 0
            if j - i > 1:
                assert pl["valid"][p] == 1 and np.isfinite(pt["cost"][p]) and np.isfinite(r.edge_cost[k, i, j - i - 1])
            coeff[s, :, :, k], durs[s, k] = seg[0, :, :, p], dts[0, p]
        n_segs[k] = len(keep) - 1
        status, mkeep, cost, chain = XM.dp(r.edge_cost[k], int(n_wp[k]), 4)
        assert mkeep == keep
        same_bits([r.cost[k], r.chain_cost[k]], [cost, chain], "programme of query %d" % k)
    assert any(len(r.keep[k]) < n_wp[k] for k in (0, 2))  # something was shortcut
    # the result holds the chosen pairs' segments: a host load of the same segments reads the same everywhere
    ref = env.load_traj(coeff, durs, n_segs=n_segs, control=m.JRK)
    live = [0, 2, 4]
    assert np.array_equal(r.poly.n_segs[live], n_segs[live]) and not r.poly.status[live].any()
    a, b = r.poly.info(want_states=True), ref.info(want_states=True)
    x, y = r.poly.sample(N=31), ref.sample(N=31)
    la, lb = r.poly.limits(all_roots=True), ref.limits(all_roots=True)
    for k in live:
        same_bits(a["effort"][:, k], b["effort"][:, k], "efforts of query %d" % k)
        same_bits(a["seg_state"][:, :, k], b["seg_state"][:, :, k], "waypoints of query %d" % k)
        same_bits(x["samples"][:, k], y["samples"][:, k], "samples of query %d" % k)
        for key in ("max_vel", "max_acc", "max_jrk"):
            same_bits(la[key][:, k], lb[key][:, k], "%s of query %d" % (key, k))
    ref.free()
    r.free()
    env.close()


def test_search_result_shortcut_end_to_end(engine):
    from test_gpu_open import corridor_env
    m = engine
    env, start, goal = corridor_env(m)
    res = env.search(start, goal, capacity=1 << 15, max_frontier=4096)
    assert res.found and res.cost == 351.5
    sc = res.shortcut()
    assert sc.status.tolist() == [0] and sc.cost[0] <= sc.chain_cost[0]
    keep = sc.keep[0]
    s0, act = res.path()
    chain = env.traj_info(s0, act.reshape(-1, 1), want_states=True)["seg_state"][:, :, 0]
    assert keep[0] == 0 and keep[-1] == len(act) and sc.poly.n_segs[0] == len(keep) - 1
    taus = sc.poly.taus()[:len(keep), 0]
    s = sc.poly.sample(times=taus[None, :], form=m.TRAJ_COMMAND)["samples"][:2, 0, :]
    assert np.abs(s - chain[:2, keep]).max() <= 1e-9
    vs = [0.5, 1.0, 2.0, 4.0]
    poly = res.smooth(v=vs)
    pick = int(m.pick_fastest(poly, 1, vs)[0])
    lim, trav = poly.limits(all_roots=True), poly.traverse()
    good = [bool(poly.status[i] == 0 and lim["valid"][i] == 1 and np.isfinite(trav["cost"][i])) for i in range(4)]
    assert pick == (max(i for i in range(4) if good[i]) if any(good) else -1), (pick, good)
    poly.free()
    sc.free()
    res.free()
    env.close()


def test_argument_errors(engine):
    import ctypes as C
    m = engine
    A, L = m._abi, m._abi.lib()
    env = m.EnvMap(2)
    pairs, res = env.alloc_poly(16, 2), env.alloc_poly(1, 5)
    st = np.ascontiguousarray(detour_chain()[:, :5])
    i, o = A.ShortcutIn(), A.ShortcutOut()
    i.states, i.n_query, i.w_max, i.control, i.stride, i.max_hop = st.ctypes.data, 1, 5, m.ACC, 1, 4
    call = lambda: L.mplx_shortcut(pairs._h, res._h, C.byref(i), C.byref(o))
    assert call() == A.ERR_STATE  # no map
    env.setMap(MAP2[1], MAP2[0], np.zeros(1600, np.int8), MAP2[2])
    env.set_v_max(2.0)
    env._flush()  # (the raw calls below go round the Python front end, which sends parameters lazily)
    assert call() == A.OK
    for key, bad in (("max_hop", 0), ("w_max", 1), ("w_max", 6), ("control", 0x0F), ("stride", 0), ("n_query", 2), ("states", None)):
        keep = getattr(i, key)
        setattr(i, key, bad)
        assert call() == A.ERR_ARG, key
        setattr(i, key, keep)
    i.max_hop = 5  # 1 x 4 x 5 = 20 pairs > 16
    assert call() == A.ERR_ARG
    i.max_hop = 4
    assert L.mplx_shortcut(pairs._h, pairs._h, C.byref(i), C.byref(o)) == A.ERR_ARG
    assert L.mplx_shortcut(pairs._h, None, C.byref(i), C.byref(o)) == A.ERR_ARG and L.mplx_shortcut(None, res._h, C.byref(i), C.byref(o)) == A.ERR_ARG
    i.n_query = 0
    assert call() == A.OK
    # the gather form of the load: src must be a filled poly of this context, not the target
    g, go = A.PolyLoadIn(), A.PolyLoadOut()
    idx = m.DeviceArray(env, 16)
    idx.upload(np.array([0, 1, -1, -1], np.int32))
    g.n_prob, g.w_max, g.control, g.src, g.src_index, g.index_stride = 1, 5, m.ACC, pairs._h.value, idx.ptr, 1
    assert L.mplx_poly_load(res._h, C.byref(g), C.byref(go)) == A.OK
    g.src = res._h.value
    assert L.mplx_poly_load(res._h, C.byref(g), C.byref(go)) == A.ERR_ARG
    g.src, g.index_stride = pairs._h.value, 0
    assert L.mplx_poly_load(res._h, C.byref(g), C.byref(go)) == A.ERR_ARG
    fresh = env.alloc_poly(4, 2)
    g.src, g.index_stride = fresh._h.value, 1
    assert L.mplx_poly_load(res._h, C.byref(g), C.byref(go)) == A.ERR_ARG  # nothing in it
    for b in (idx, fresh, pairs, res):
        b.free()
    env.close()
