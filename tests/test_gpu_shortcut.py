"""mplx_shortcut on the device (include/mplx_limits.h, csrc/limits_kernel.hip) against tests/shortcut_model.py.

The first four tests run one query (Q = 5 for the invariants): ACC in 2-D bit for bit (edge costs from the pair
coefficients the device returned, then the programme), JRK in 3-D on a potential map held to invariants, a search result
end to end, the argument errors.

THE BATCH (shortcut_model.batch, one cached input set per dimension): Q = 67 queries, w_max = 6, max_hop = 3, hence 1005
pairs -- four blocks of the pair and cost kernels, the last one partial, and two blocks (waves) of the solve and of the
gather.  n_wp[k] = k % 8: k % 8 < 2 is EMPTY, k % 8 == 7 is above w_max and behaves as 6.  States [4D+2][6][67]: random
short paths on the map, velocities / accelerations / jerks rounded to 1/100, a yaw per state, t strictly increasing in
unequal multiples of 1/8.  2-D: 40 x 40 cells of 0.25 with a wall at x in [4.75, 5.25), y < 6; 3-D: 24 x 21 x 19 cells
with a slab at x in [1.75, 2.25), y < 3.5, and for ACC / JRK a random potential map (100 in the slab).  Which k is what:
    k = 6, 63   TIE: six states one metre and one second apart on a free line, vel = 1.  Under VEL every hop of length h
                costs exactly 11 h (J = h, w T = 10 h, no potential map), every chain ties, and "ties to the smallest i"
                keeps [0, 2, 5] (63 has n_wp = 7: the clamp, with a known answer)
    k = 14      REPEATED T: t_3 == t_2, so pair (2, 3) is BAD_TIME and the query BAD_CHAIN: the identity chain, NaN costs
    k = 22      WALL: the same line through the wall between states 2 and 3: the piece 2 -> 3 is admitted with its
                traversal counted as 0.0, every hop over it is +inf, keep = [0, 2, 3, 5]
    k = 66      WALL with W = 2, in the second wave: its only piece goes through the wall
    k = 30      OFF THE MAP: state 3 lies past the map's edge: the pieces 2 -> 3 -> 4 are admitted, hops from or to 3 +inf
n_wp[k] = k % 8 leaves lanes 64 .. 66 with W = 0, 1, 2, so of the special kinds the second wave sees EMPTY and WALL only;
the others need W = 6 and sit below 64.

Eight configurations (CONFIGS): VEL, ACC, JRK in 2-D, VEL in 3-D, ACC and JRK in 3-D on the potential map, ACCxYAW in
2-D, JRKxYAW in 3-D on the potential map.  Per configuration the device runs once (run()); the four tests read it:
  (a) test_batch_pairs     every pair with j < W_k joins state i to state j of query k, whatever the device's coefficients
                           are: status 0 iff t_j - t_i is finite and > 0, the duration the one IEEE subtraction, the two
                           waypoints of the pair the two states bit for bit, the yaw solve bit for bit, the coefficients
                           bit for bit for VEL and under the rule of tests/test_gpu_solve.py for ACC / JRK
                           (check_against_bound: e_dev <= 8 max(e_ref, 2^-52 scale) against solve_exact); pairs with
                           j >= W_k are SOLVE_EMPTY.  All 1005.
  (b) test_batch_edge_costs  bit for bit shortcut_model.edge_costs (the yaw bit included: it adds nothing to validity and
                           the effort row is the control's own).  JRK only: a non-adjacent pair may be left out when a
                           model ALL_ROOTS maximum of a checked limit lies within a relative 1e-9 of it (the decision then
                           turns on the device library's cbrt / acos / cos); at most 2 % of the pairs, the count printed.
  (c) test_batch_programme  status, keep, cost, chain_cost bit for bit shortcut_model.dp on the device's own edge costs;
                           raw keep rows past n_keep are -1; at least a fifth of the live queries shortcut something and
                           at least a fifth keep an interior state.
  (d) test_batch_result    the result poly is the chosen pairs: n_segs, taus (sequential sums of the pairs' durations),
                           and -- the segment table of a gathered poly cannot be read back -- efforts, waypoints, total
                           time and 25 samples bit for bit those of EnvMap.load_traj of the chosen pairs' segments;
                           waypoint s is chain state keep[s] in the derivative rows the order fixes, within the bound of
                           (a) propagated through the polynomial; BAD_CHAIN and EMPTY queries are SOLVE_EMPTY problems.
Raw ABI (ACC, 2-D): the host twin with stride 71, keep_stride 73 and poisoned outputs equals the device form bit for bit
and leaves the padding alone, with and without n_wp; the device form with the same strides, then with every output NULL;
three calls on one pair of polys (Q = 67 / hop 3, Q = 5 / hop 5, the first again).  MultiSearchResult.shortcut against
EnvMap.shortcut of each query's own chain states."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import shortcut_model as XM
import solve_model as SM
from test_gpu_solve import EPS, FACTOR, check_against_bound, same_bits

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


# ---------------------------------------------------------------------------------------------------------- the batch
CONFIGS = {"vel-2d": (2, 0x01), "vel-3d": (3, 0x01), "acc-2d": (2, 0x03), "acc-3d-pot": (3, 0x03), "jrk-2d": (2, 0x07),
           "jrk-3d-pot": (3, 0x07), "accyaw-2d": (2, 0x13), "jrkyaw-3d-pot": (3, 0x17)}
Q, WMAX, HOP = XM.Q, XM.WMAX, XM.HOP
NP = Q * (WMAX - 1) * HOP
N_SAMPLES = 24
POISON = 0xA5


def batch_env(m, D, control):
    b = XM.batch(D, control)
    md, org, res = b["map"]
    env = m.EnvMap(D)
    env.setMap(org, md, b["grid"], res)
    env.set_control(control & 0x0F)
    env.set_v_max(b["v_max"])
    env.set_a_max(b["a_max"])
    env.set_w(XM.W_TIME)
    env.set_potential_weight(XM.POT_W)
    env.set_gradient_weight(XM.GRAD_W)
    if b["pot"] is not None:
        env.set_potential_map(b["pot"])
    return env


class HeldPairs:
    """The rows of a pair set after its poly was freed (what shortcut_model.edge_costs reads)."""

    def __init__(self, pairs):
        self.n, self.status = pairs.n, pairs.status.copy()
        self._rows = (pairs.coefficients().copy(), pairs.yaw_coefficients().copy(), pairs.dts().copy())
        self.segs = pairs.segments().copy()
        self.states = pairs.info(want_states=True)["seg_state"]

    def coefficients(self):
        return self._rows[0]

    def yaw_coefficients(self):
        return self._rows[1]

    def dts(self):
        return self._rows[2]


def chosen_segments(D, keep_lists, pairs, w_max, hop):
    """(coeff [w_max - 1][D + 1][6][Q], durs, n_segs) of EnvMap.load_traj: per query the segments of its chosen pairs."""
    n = len(keep_lists)
    coeff, durs, n_segs = np.zeros((w_max - 1, D + 1, 6, n)), np.ones((w_max - 1, n)), np.zeros(n, np.int32)
    for k, keep in enumerate(keep_lists):
        ps = [XM.pair_index(k, i, j, w_max, hop) for i, j in zip(keep, keep[1:])]
        if not ps or pairs.status[ps].any():
            continue
        for s, p in enumerate(ps):
            coeff[s, :, :, k], durs[s, k] = pairs.segs[0, :, :, p], pairs.dts()[0, p]
        n_segs[k] = len(ps)
    return coeff, durs, n_segs


_RUNS = {}


def run(m, name):
    """One EnvMap.shortcut of the batch per configuration, everything the tests read brought to the host, the device
    objects freed: the outputs, the pair set, the result poly and its twin (a load of the chosen pairs' segments)."""
    if name not in _RUNS:
        D, control = CONFIGS[name]
        b = XM.batch(D, control)
        env = batch_env(m, D, control)
        r = env.shortcut(b["states"], n_wp=b["n_wp"], control=control, max_hop=HOP)
        out = {"status": r.status, "n_keep": r.n_keep, "keep_rows": r.keep_rows, "keep": [k.tolist() for k in r.keep],
               "cost": r.cost, "chain_cost": r.chain_cost, "edge_cost": r.edge_cost, "pairs": HeldPairs(r.pairs)}
        out["poly"] = {"status": r.poly.status.copy(), "n_segs": r.poly.n_segs.copy(), "taus": r.poly.taus().copy(),
                       "info": r.poly.info(want_states=True), "samples": r.poly.sample(N=N_SAMPLES)}
        coeff, durs, n_segs = chosen_segments(D, out["keep"], out["pairs"], WMAX, HOP)
        twin = env.load_traj(coeff, durs, n_segs=n_segs, control=control)
        out["twin"] = {"status": twin.status.copy(), "n_segs": n_segs, "info": twin.info(want_states=True),
                       "samples": twin.sample(N=N_SAMPLES)}
        twin.free()
        r.free()
        env.close()
        _RUNS[name] = out
    return _RUNS[name]


@functools.lru_cache(maxsize=None)
def pair_reference(D, so):
    """Per pair with j < W_k and a duration > 0: (dense, exact or None (so = 0), yaw, e_ref, scale) of its two-waypoint
    problem; computed once per (D, so) and shared by (a) and (d)."""
    st, n_wp = XM.batch_states(D)
    ref = {}
    for k in range(Q):
        W = XM.w_of(n_wp, k)
        for i in range(W - 1):
            for j in range(i + 1, min(i + HOP, W - 1) + 1):
                vals, flags, dts, yaw = XM.pair_problem(st, k, i, j, D)
                if not (np.isfinite(dts[0]) and dts[0] > 0):
                    continue
                dense = SM.solve_dense(vals, flags, dts, so)
                exact = SM.solve_exact(vals, flags, dts, so) if so else None
                e_ref, scale = (SM.max_err(dense, exact), SM.scale_of(exact)) if so else (0.0, float(np.abs(dense).max()))
                ref[XM.pair_index(k, i, j, WMAX, HOP)] = (dense, exact, SM.yaw_solve(yaw, dts)[:, 0], e_ref, scale)
    return ref


@pytest.mark.parametrize("name", list(CONFIGS))
def test_batch_pairs(engine, name):
    """(a) of the module's docstring."""
    m = engine
    D, control = CONFIGS[name]
    b, r = XM.batch(D, control), run(engine, name)
    st, n_wp, so, pairs = b["states"], b["n_wp"], b["so"], r["pairs"]
    ref = pair_reference(D, so)
    coef, yaw, pdts = pairs.coefficients(), pairs.yaw_coefficients(), pairs.dts()
    assert pairs.n == NP and coef.shape == (1, 2 * (so + 1), D, NP)
    worst, solved = 0.0, 0
    for k in range(Q):
        W = XM.w_of(n_wp, k)
        for i in range(WMAX - 1):
            for j in range(i + 1, i + HOP + 1):
                p = XM.pair_index(k, i, j, WMAX, HOP)
                what = "pair %d = (k %d, %d -> %d)" % (p, k, i, j)
                if j >= W:
                    assert pairs.status[p] == m.SOLVE_EMPTY, what
                    continue
                dt = st[4 * D + 1, j, k] - st[4 * D + 1, i, k]
                if not (np.isfinite(dt) and dt > 0):
                    assert pairs.status[p] == m.SOLVE_BAD_TIME and p not in ref, what
                    continue
                assert pairs.status[p] == 0, what
                solved += 1
                same_bits([pdts[0, p]], [dt], "duration of " + what)
                same_bits(pairs.states[:, 0, p], st[:, i, k], "first waypoint of " + what)
                same_bits(pairs.states[:, 1, p], st[:, j, k], "second waypoint of " + what)
                dense, exact, yaw_p, _, _ = ref[p]
                same_bits(yaw[0, :, p], yaw_p, "yaw coefficients of " + what)
                if so == 0:
                    same_bits(coef[0, :, :, p], dense, "coefficients of " + what)
                else:
                    worst = max(worst, check_against_bound(coef[0, :, :, p], dense, exact, what))
    assert solved == len(ref) and solved > 300
    print("%s: %d pairs solved, worst e_dev / max(e_ref, eps scale) = %.3f" % (name, solved, worst))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_batch_edge_costs(engine, name):
    """(b) of the module's docstring."""
    D, control = CONFIGS[name]
    b, r = XM.batch(D, control), run(engine, name)
    so, pairs = b["so"], r["pairs"]
    want, near, trav = XM.edge_costs(pairs, HOP, D, so, control, XM.W_TIME, b["limits"], b["world"], want_detail=True)
    got = r["edge_cost"].reshape(-1)
    assert r["edge_cost"].shape == (Q, WMAX - 1, HOP) and not near[::HOP].any()
    left_out = near if so == 2 else np.zeros(NP, bool)
    print("%s: %d of %d pairs left out (a checked maximum within %g of its limit)" % (name, left_out.sum(), NP, XM.NEAR))
    assert left_out.sum() <= 0.02 * NP
    same_bits(got[~left_out], want[~left_out], "edge costs")
    # the branches no other device test reaches: an adjacent piece whose traversal is not finite counts it as 0.0
    c, trav = r["edge_cost"], trav.reshape(Q, WMAX - 1, HOP)
    for k, i in ((XM.WALL[0], 2), (XM.WALL[1], 0), (XM.OFF_MAP[0], 2), (XM.OFF_MAP[0], 3)):
        assert np.isinf(trav[k, i, 0]) and np.isfinite(c[k, i, 0]), (k, i)
    k = XM.WALL[0]
    assert np.isinf([c[k, 0, 2], c[k, 1, 1], c[k, 1, 2], c[k, 2, 1], c[k, 2, 2]]).all()
    k = XM.OFF_MAP[0]
    assert np.isinf([c[k, 0, 2], c[k, 1, 1], c[k, 3, 1]]).all() and np.isfinite(c[k, 2, 1])
    for k in XM.REPEAT_T:
        assert np.isnan(c[k, 2, 0]) and not pairs.status[XM.pair_index(k, 1, 3, WMAX, HOP)]  # (the hop over it is solved)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_batch_programme(engine, name):
    """(c) of the module's docstring."""
    m = engine
    D, control = CONFIGS[name]
    b, r = XM.batch(D, control), run(engine, name)
    n_wp, c = b["n_wp"], r["edge_cost"]
    live = []
    for k in range(Q):
        W = XM.w_of(n_wp, k)
        status, keep, cost, chain = XM.dp(c[k], W, HOP)
        assert r["status"][k] == status and r["keep"][k] == keep and r["n_keep"][k] == len(keep), (k, r["keep"][k], keep)
        assert r["keep_rows"][:len(keep), k].tolist() == keep and (r["keep_rows"][len(keep):, k] == -1).all(), k
        same_bits([r["cost"][k], r["chain_cost"][k]], [cost, chain], "cost and chain_cost of query %d" % k)
        if k % 8 < 2:
            assert status == m.SOLVE_EMPTY and r["n_keep"][k] == 0 and np.isnan(r["cost"][k]) and np.isnan(r["chain_cost"][k])
        elif k in XM.REPEAT_T:
            assert status == m.SHORTCUT_BAD_CHAIN and keep == list(range(W)) and np.isnan(r["cost"][k]) and np.isnan(r["chain_cost"][k])
        else:
            assert status == 0 and keep[0] == 0 and keep[-1] == W - 1 and r["cost"][k] <= r["chain_cost"][k], k
            live.append(k)
    assert r["keep"][XM.WALL[0]] == [0, 2, 3, 5] and r["keep"][XM.WALL[1]] == [0, 1]
    if control == m.VEL:
        for k in XM.TIE:  # first the premise -- every hop of length h costs exactly 11 h --, then the known answer
            for i in range(WMAX - 1):
                for h in range(min(HOP, WMAX - 1 - i)):
                    assert c[k, i, h] == 11.0 * (h + 1), (k, i, h, c[k, i, h])
            assert r["keep"][k] == [0, 2, 5] and r["cost"][k] == 55.0 and r["chain_cost"][k] == 55.0, (k, r["keep"][k])
    short = sum(len(r["keep"][k]) < XM.w_of(n_wp, k) for k in live)
    interior = sum(len(r["keep"][k]) > 2 for k in live)
    print("%s: %d live queries, %d shortcut something, %d keep an interior state" % (name, len(live), short, interior))
    assert len(live) == 48 and 5 * short >= len(live) and 5 * interior >= len(live)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_batch_result(engine, name):
    """(d) of the module's docstring."""
    m = engine
    D, control = CONFIGS[name]
    b, r = XM.batch(D, control), run(engine, name)
    st, so, pairs, poly, twin = b["states"], b["so"], r["pairs"], r["poly"], r["twin"]
    ref = pair_reference(D, so)
    N, fact = 2 * (so + 1), [1.0, 1.0, 2.0, 6.0, 24.0, 120.0]
    a, t = poly["info"], twin["info"]
    for k in range(Q):
        keep = r["keep"][k]
        if r["status"][k]:  # EMPTY, and BAD_CHAIN (the identity chain holds the failed pair: nothing to gather)
            assert poly["status"][k] == m.SOLVE_EMPTY and poly["n_segs"][k] == 0 and a["status"][k] == m.SOLVE_EMPTY, k
            assert not poly["samples"]["samples"][:, k].any() and poly["samples"]["status"][k] == m.SOLVE_EMPTY, k
            continue
        S = len(keep) - 1
        ps = [XM.pair_index(k, i, j, WMAX, HOP) for i, j in zip(keep, keep[1:])]
        assert poly["status"][k] == 0 and poly["n_segs"][k] == S and twin["status"][k] == 0 and twin["n_segs"][k] == S, k
        same_bits(poly["taus"][:S + 1, k], SM.set_time(pairs.dts()[0, ps]), "taus of query %d" % k)
        same_bits([a["total_time"][k]], [t["total_time"][k]], "total time of query %d" % k)
        same_bits(a["effort"][:, k], t["effort"][:, k], "efforts of query %d" % k)
        same_bits(a["seg_state"][:, :, k], t["seg_state"][:, :, k], "waypoints of query %d" % k)
        same_bits(poly["samples"]["samples"][:, k], twin["samples"]["samples"][:, k], "samples of query %d" % k)
        # waypoint s is chain state keep[s]: the start of segment s (the end of the last one).  A coefficient error of at
        # most B = FACTOR max(e_ref, eps scale), the bound of (a), moves derivative r at time T by at most B A_r with A_r =
        # sum_n n! / (n - r)! T^(n - r); evaluating the polynomial rounds each of its <= 6 terms at most 7 times and the
        # partial sums 5 times, all below scale A_r: 16 eps scale A_r; and one ulp of the state itself
        for s in range(S + 1):
            p = ps[min(s, S - 1)]
            _, _, _, e_ref, scale = ref[p]
            T = max(float(pairs.dts()[0, p]), 1.0)
            for d in range(so + 1):
                A = sum(fact[n] / fact[n - d] * T ** (n - d) for n in range(d, N))
                want = st[d * D:(d + 1) * D, keep[s], k]
                tol = FACTOR * max(e_ref, EPS * scale) * A + 16 * EPS * scale * A + EPS * np.abs(want).max()
                err = np.abs(a["seg_state"][d * D:(d + 1) * D, s, k] - want).max()
                assert err <= tol, (k, s, d, err, tol)


# ------------------------------------------------------------------------------------------------------ the raw ABI
ROWS = ("status", "n_keep", "keep", "cost", "chain_cost", "edge_cost")


def raw_shortcut(m, env, pairs, res, st, n_wp, control, hop, device, stride=None, keep_stride=None, outputs=True, pair_out=False):
    """mplx_shortcut (device=False) or mplx_shortcut_device on outputs filled with the byte POISON; states padded to
    `stride` with NaN columns, the [Q] rows and the columns of keep `keep_stride` long, edge_cost eight entries longer than
    its pairs.  Returns (rc, rows as they came back or None, the result poly's samples)."""
    import ctypes as C
    A, L = m._abi, m._abi.lib()
    env._flush()  # (the raw calls go round the Python front end, which sends parameters lazily)
    Fd, W, n = st.shape
    stride, ks, P = stride or n, keep_stride or n, n * (W - 1) * hop
    padded = np.full((Fd, W, stride), np.nan)
    padded[:, :, :n] = st
    shapes = {"status": ((ks,), np.uint8), "n_keep": ((ks,), np.int32), "keep": ((W, ks), np.int32), "cost": ((ks,), np.float64),
              "chain_cost": ((ks,), np.float64), "edge_cost": ((P + 8,), np.float64)}
    host = {key: np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, POISON, np.uint8).view(dt).reshape(shape)
            for key, (shape, dt) in shapes.items()}
    i, o = A.ShortcutIn(), A.ShortcutOut()
    i.n_query, i.w_max, i.control, i.stride, i.max_hop = n, W, control, stride, hop
    o.keep_stride = ks if outputs else 0
    if pair_out:
        po = A.SolveOut()
        o.pair_out = C.pointer(po)
    bufs = {}
    try:
        if device:
            for key, arr in [("states", padded)] + ([("n_wp", np.ascontiguousarray(n_wp, np.int32))] if n_wp is not None else []):
                bufs[key] = m.DeviceArray(env, arr.nbytes)
                bufs[key].upload(arr)
                setattr(i, key, bufs[key].ptr)
            for key in ROWS if outputs else ():
                bufs[key] = m.DeviceArray(env, host[key].nbytes)
                A.check(env._ctx, L.mplx_memset(env._ctx, bufs[key].ptr, POISON, host[key].nbytes))
                setattr(o, key, bufs[key].ptr)
            rc = L.mplx_shortcut_device(pairs._h, res._h, C.byref(i), C.byref(o))
            env.synchronize()
            for key in ROWS if outputs and rc == A.OK else ():
                host[key] = bufs[key].download(shapes[key][1], shapes[key][0])
        else:
            i.states = padded.ctypes.data
            if n_wp is not None:
                n_wp = np.ascontiguousarray(n_wp, np.int32)
                i.n_wp = n_wp.ctypes.data
            for key in ROWS if outputs else ():
                setattr(o, key, host[key].ctypes.data)
            rc = L.mplx_shortcut(pairs._h, res._h, C.byref(i), C.byref(o))
    finally:
        for buf in bufs.values():
            buf.free()
    if rc != A.OK:
        return rc, None, None
    res.n, res.n_wmax, res.control = n, W, control
    return rc, (host if outputs else None), res.sample(N=N_SAMPLES)["samples"]


def poison(a):
    return (np.ascontiguousarray(a).view(np.uint8) == POISON).all()


def assert_rows_equal(rows, want, n, P, what):
    """rows: raw_shortcut's, with strides; want: dict of compact rows ([n], keep [W][n], edge_cost [P])."""
    for key in ROWS:
        got = rows[key]
        body, tail = (got[:P], got[P:]) if key == "edge_cost" else (got[..., :n], got[..., n:])
        assert np.array_equal(np.ascontiguousarray(body).view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8)), (what, key)
        assert tail.size > 0 and poison(tail), (what, key, "the padding was written")


def compact(r):
    return {"status": r["status"], "n_keep": r["n_keep"], "keep": r["keep_rows"], "cost": r["cost"], "chain_cost": r["chain_cost"],
            "edge_cost": r["edge_cost"].reshape(-1)}


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_raw_strides_and_untouched_memory(engine, device):
    """(e) and (f): the host twin and the device form on the ACC 2-D batch with stride 71, keep_stride 73 and poisoned
    outputs: bit for bit what EnvMap.shortcut (the device form, compact) returned, the padding untouched; the same without
    n_wp (every query W = 6) against a device call with n_wp = 6 everywhere; then every output NULL (the kernel's own
    edge-cost scratch row): the same result trajectories; pair_out is for the device form only."""
    m, A = engine, engine._abi
    D, control = CONFIGS["acc-2d"]
    b, want = XM.batch(D, control), run(engine, "acc-2d")
    st = b["states"]
    env = batch_env(m, D, control)
    pairs, res = env.alloc_poly(NP, 2), env.alloc_poly(Q, WMAX)
    rc, rows, samples = raw_shortcut(m, env, pairs, res, st, b["n_wp"], control, HOP, device, stride=71, keep_stride=73)
    assert rc == A.OK
    assert_rows_equal(rows, compact(want), Q, NP, "with n_wp")
    assert same_bytes(samples, want["poly"]["samples"]["samples"])
    rc, none, samples2 = raw_shortcut(m, env, pairs, res, st, b["n_wp"], control, HOP, device, stride=71, outputs=False)
    assert rc == A.OK and none is None and same_bytes(samples2, samples)
    full = env.shortcut(st, n_wp=np.full(Q, WMAX, np.int32), control=control, max_hop=HOP)
    assert full.status.tolist() == [m.SHORTCUT_BAD_CHAIN if k in XM.REPEAT_T else 0 for k in range(Q)] and (full.n_keep >= 2).all()
    rc, rows, samples = raw_shortcut(m, env, pairs, res, st, None, control, HOP, device, stride=71, keep_stride=73)
    assert rc == A.OK
    assert_rows_equal(rows, {"status": full.status, "n_keep": full.n_keep, "keep": full.keep_rows, "cost": full.cost,
                             "chain_cost": full.chain_cost, "edge_cost": full.edge_cost.reshape(-1)}, Q, NP, "without n_wp")
    assert same_bytes(samples, full.poly.sample(N=N_SAMPLES)["samples"])
    rc, _, _ = raw_shortcut(m, env, pairs, res, st, b["n_wp"], control, HOP, device, stride=71, keep_stride=73, pair_out=True)
    assert rc == (A.OK if device else A.ERR_ARG)  # (an all-NULL pair_out is a valid one for the device form)
    for x in (full, pairs, res):
        x.free()
    env.close()


def test_raw_reuse_of_the_polys(engine):
    """(g): one pair poly and one result poly through the batch (Q = 67, max_hop 3), then Q = 5 with max_hop = 5 (above
    W_k - 1 for the chains of 2 .. 5 states; the scratch block of the pair poly is carved anew, smaller), then the batch
    again: call 3 is call 1 bit for bit, call 2 is the same call on fresh polys."""
    m, A = engine, engine._abi
    D, control = CONFIGS["acc-2d"]
    b = XM.batch(D, control)
    st, n_wp = b["states"], b["n_wp"]
    st2, n_wp2 = np.ascontiguousarray(st[:, :, 2:7]), n_wp[2:7]
    assert n_wp2.tolist() == [2, 3, 4, 5, 6]
    env = batch_env(m, D, control)
    pairs, res = env.alloc_poly(NP, 2), env.alloc_poly(Q, WMAX)
    big = lambda: raw_shortcut(m, env, pairs, res, st, n_wp, control, HOP, True, stride=71, keep_stride=73)
    small = lambda ps, rs: raw_shortcut(m, env, ps, rs, st2, n_wp2, control, 5, True, stride=7, keep_stride=9)
    one, two, three = big(), small(pairs, res), big()
    fresh_pairs, fresh_res = env.alloc_poly(125, 2), env.alloc_poly(5, WMAX)
    fresh = small(fresh_pairs, fresh_res)
    for got, want, what in ((three, one, "the batch again"), (two, fresh, "the small call")):
        assert got[0] == A.OK and want[0] == A.OK
        for key in ROWS:
            assert same_bytes(got[1][key], want[1][key]), (what, key)
        assert same_bytes(got[2], want[2]), (what, "samples")
    assert_rows_equal(one[1], compact(run(engine, "acc-2d")), Q, NP, "the batch")
    rows = two[1]
    assert rows["status"][:5].tolist() == [0] * 5 and rows["keep"][:2, 0].tolist() == [0, 1]
    for k in range(5):  # max_hop = 5 > W_k - 1: the hops past the chain are empty pairs, +inf
        c = rows["edge_cost"][:125].reshape(5, 5, 5)[k]
        W = int(n_wp2[k])
        status, keep, cost, chain = XM.dp(c, W, 5)
        assert rows["keep"][:rows["n_keep"][k], k].tolist() == keep and (rows["keep"][rows["n_keep"][k]:, k] == -1).all()
        same_bits([rows["cost"][k], rows["chain_cost"][k]], [cost, chain], "programme of the small call, query %d" % k)
        assert all(np.isinf(c[i, h]) for i in range(W - 1) for h in range(1, 5) if i + h + 1 >= W)
    for x in (pairs, res, fresh_pairs, fresh_res):
        x.free()
    env.close()


def test_multi_search_result_shortcut(engine):
    """(h): MultiSearchResult.shortcut on the corridor's four queries (one batch of launches) against EnvMap.shortcut of
    each query's own chain states, bit for bit; the context searches afterwards as before.  The four paths all have 36
    states, so a fifth query starts from chain state 12 of the first one: a shorter chain, padded in the batch."""
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    m = engine
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    starts = np.concatenate([starts, starts[:, 1:2]], axis=1)  # a fourth query: the shifted start to the original goal
    goals = np.concatenate([goals, goals[0:1]])
    kw = dict(eps=1.0, delta=10.0, capacity=1 << 16)
    first = env.search_many(starts, goals, **kw)
    s0, act = first.path(0)
    mid = env.traj_info(s0, act.reshape(-1, 1), want_states=True)["seg_state"][:, 12, 0].copy()
    mid[-1] = 0.0  # (its clock starts anew)
    first.free()
    starts, goals = np.concatenate([starts, mid[:, None]], axis=1), np.concatenate([goals, goals[0:1]])
    multi = env.search_many(starts, goals, **kw)
    assert multi.found == [True] * 5
    hop = 4
    sc = multi.shortcut(max_hop=hop)
    lengths = [len(multi.path(q)[1]) + 1 for q in range(5)]
    print("chain states per query:", lengths)
    assert len(set(lengths)) > 1 and sc.edge_cost.shape == (5, max(lengths) - 1, hop) and not sc.status.any()
    all_samples = sc.poly.sample(N=N_SAMPLES)["samples"]
    for q in range(5):
        s0, act = multi.path(q)
        chain = env.traj_info(s0, act.reshape(-1, 1), want_states=True)["seg_state"][:, :, 0]
        W = lengths[q]
        assert chain.shape[1] == W
        one = env.shortcut(chain[:, :, None], max_hop=hop)
        assert one.status.tolist() == [0] and sc.keep[q].tolist() == one.keep[0].tolist(), q
        assert (sc.keep_rows[len(sc.keep[q]):, q] == -1).all()
        same_bits([sc.cost[q], sc.chain_cost[q]], [one.cost[0], one.chain_cost[0]], "costs of query %d" % q)
        same_bits(sc.edge_cost[q, :W - 1], one.edge_cost[0], "edge costs of query %d" % q)
        assert np.isinf(sc.edge_cost[q, W - 1:, 1:]).all() and np.isnan(sc.edge_cost[q, W - 1:, 0]).all()  # past the chain
        assert sc.poly.n_segs[q] == one.poly.n_segs[0] == len(one.keep[0]) - 1
        same_bits(all_samples[:, q], one.poly.sample(N=N_SAMPLES)["samples"][:, 0], "samples of query %d" % q)
        assert len(one.keep[0]) < W  # something was shortcut
        one.free()
    sc.free()
    again = env.search_many(starts, goals, **kw)  # the context is as it was
    assert again.cost == multi.cost and again.expanded == multi.expanded and again.rounds == multi.rounds
    for q in range(5):
        assert np.array_equal(again.path(q)[1], multi.path(q)[1])
    again.free()
    multi.free()
    env.close()
