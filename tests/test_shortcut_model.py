"""tests/shortcut_model.py: the dynamic programme against a brute force over every chain of hops (no GPU).  The costs are
multiples of 1/8 below 2^10, so every sum is exact and ties are real ties; +inf marks hops that are not admitted."""
import numpy as np
import pytest

import shortcut_model as XM


def matrix(rng, W, max_hop, p_inf, levels):
    c = rng.integers(1, levels, (W - 1, max_hop)).astype(np.float64) / 8.0
    c[rng.random(c.shape) < p_inf] = np.inf
    c[:, 0] = rng.integers(1, levels, W - 1) / 8.0  # the adjacent hop is always admitted
    return c


@pytest.mark.parametrize("W", [2, 3, 5, 8])
def test_dp_equals_brute_force(W):
    rng = np.random.default_rng(40 + W)
    for trial in range(60):
        max_hop = int(rng.integers(1, W + 1))
        c = matrix(rng, W, max_hop, 0.3 * (trial % 3), 4 if trial % 2 else 64)  # few levels: many exact ties
        status, keep, cost, chain = XM.dp(c, W, max_hop)
        want_keep, want_cost = XM.brute(c, W, max_hop)
        assert status == 0 and keep == want_keep, (W, trial, keep, want_keep)
        assert np.float64(cost).view(np.uint64) == np.float64(want_cost).view(np.uint64)
        assert keep[0] == 0 and keep[-1] == W - 1 and cost <= chain
        assert chain == sum(c[:, 0])
        if max_hop == 1:
            assert keep == list(range(W)) and cost == chain


def test_ties_go_to_the_smallest_predecessor():
    c = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, np.inf], [1.0, np.inf, np.inf]])  # 0-3 direct, 0-1-3, 0-2-3, 0-1-2-3: all 3
    assert XM.dp(c, 4, 3)[1] == [0, 3]
    c[0, 2] = np.inf
    assert XM.dp(c, 4, 3)[1] == [0, 1, 3]  # predecessors 1 and 2 tie: the smaller
    assert XM.brute(c, 4, 3)[0] == [0, 1, 3]


def test_statuses():
    c = np.ones((3, 2))
    assert XM.dp(c, 1, 2)[0] == XM.EMPTY and XM.dp(c, 0, 2)[0] == XM.EMPTY
    c[1, 0] = np.nan
    status, keep, cost, chain = XM.dp(c, 4, 2)
    assert status == XM.BAD_CHAIN and keep == [0, 1, 2, 3] and np.isnan(cost) and np.isnan(chain)
    assert XM.dp(c, 2, 2)[0] == 0  # the bad hop is past this chain's end


def test_every_chain_ties_known_answer():
    """Every hop of length h costs 11 h (the tie queries of the device batch): all chains tie, and "ties to the smallest
    i" keeps [0, 2, 5] for W = 6, max_hop = 3.  The brute force agrees (its tie rule is the programme's for exact sums)."""
    c = np.array([[11.0 * (h + 1) for h in range(3)] for _ in range(5)])
    status, keep, cost, chain = XM.dp(c, 6, 3)
    assert (status, keep, cost, chain) == (0, [0, 2, 5], 55.0, 55.0)
    assert XM.brute(c, 6, 3) == ([0, 2, 5], 55.0)


@pytest.mark.parametrize("D,control", sorted(XM.CONFIGS), ids=["%dD-%#x" % c for c in sorted(XM.CONFIGS)])
def test_batch_has_every_special_query(D, control):
    """The device batch (tests/test_gpu_shortcut.py) on solve_dense coefficients: every special query is what its name
    says, the programme has something to decide, and the pairs a JRK comparison may leave out stay under the 2 % cap."""
    b = XM.batch(D, control)
    st, n_wp, so = b["states"], b["n_wp"], b["so"]
    md, org, res = b["map"]
    assert st.shape == (4 * D + 2, XM.WMAX, XM.Q) and n_wp.tolist() == [k % 8 for k in range(XM.Q)]
    t = st[4 * D + 1]
    plain = [k for k in range(XM.Q) if k not in XM.REPEAT_T]
    assert (np.diff(t[:, plain], axis=0) > 0).all() and (t * 8 == np.round(t * 8)).all()
    assert len({tuple(np.diff(t[:, k])) for k in plain}) > 20  # unequal steps
    on_map = [k for k in range(XM.Q) if k not in XM.OFF_MAP]
    lo, hi = np.asarray(org)[:, None, None], (np.asarray(org) + np.asarray(md) * res)[:, None, None]
    assert (st[:D][:, :, on_map] >= lo).all() and (st[:D][:, :, on_map] < hi).all()
    pairs = XM.DensePairs(st, n_wp, D, so, XM.HOP)
    c, near, trav = XM.edge_costs(pairs, XM.HOP, D, so, control, XM.W_TIME, b["limits"], b["world"], want_detail=True)
    c, trav = c.reshape(XM.Q, XM.WMAX - 1, XM.HOP), trav.reshape(XM.Q, XM.WMAX - 1, XM.HOP)
    assert near.sum() <= 0.02 * pairs.n or so < 2, near.sum()
    out = [XM.dp(c[k], XM.w_of(n_wp, k), XM.HOP) for k in range(XM.Q)]
    for k in range(XM.Q):
        want = XM.EMPTY if k % 8 < 2 else (XM.BAD_CHAIN if k in XM.REPEAT_T else 0)
        assert out[k][0] == want, k
    for k in XM.REPEAT_T:
        # the piece 2 -> 3 has dt == 0, the hop 1 -> 3 over it has not
        assert np.isnan(c[k, 2, 0]) and pairs.status[XM.pair_index(k, 2, 3, XM.WMAX, XM.HOP)] and not pairs.status[XM.pair_index(k, 1, 3, XM.WMAX, XM.HOP)]
    k = XM.WALL[0]  # the piece 2 -> 3 goes through the wall: admitted, its traversal counted as 0.0; every hop over it +inf
    assert np.isinf(trav[k, 2, 0]) and np.isfinite(c[k, 2, 0]) and out[k][1] == [0, 2, 3, 5]
    assert np.isinf([c[k, 0, 2], c[k, 1, 1], c[k, 1, 2], c[k, 2, 1], c[k, 2, 2]]).all()
    k = XM.WALL[1]
    assert np.isinf(trav[k, 0, 0]) and np.isfinite(c[k, 0, 0]) and out[k][1] == [0, 1]
    k = XM.OFF_MAP[0]  # state 3 is off the map: the pieces 2 -> 3 -> 4 are admitted, the hops that end or start there are not
    assert np.isinf(trav[k, 2:4, 0]).all() and np.isfinite(c[k, 2:4, 0]).all()
    assert np.isinf([c[k, 0, 2], c[k, 1, 1], c[k, 3, 1]]).all() and np.isfinite(c[k, 2, 1])
    if control == 0x01:
        for k in XM.TIE:
            assert (c[k] == 11.0 * (np.arange(3) + 1.0)[None, :])[np.isfinite(c[k])].all() and np.isfinite(c[k]).sum() == 12
            assert out[k][1] == [0, 2, 5]
    live = [k for k in range(XM.Q) if out[k][0] == 0]
    assert sum(len(out[k][1]) < XM.w_of(n_wp, k) for k in live) * 5 >= len(live)
    assert sum(len(out[k][1]) > 2 for k in live) * 5 >= len(live)


@pytest.mark.parametrize("D,so", [(2, 0), (2, 1), (3, 2)])
def test_pair_problem_joins_the_two_states(D, so):
    """solve_dense of pair_problem(k, i, j) is at state i at time 0 and at state j at time T = t_j - t_i in every
    derivative the order fixes (rounding of the solve and of the evaluation: 1e-12 on values of order 1)."""
    import solve_model as SM
    import traj_model as TM
    st, n_wp = XM.batch_states(D)
    for k, i, j in ((5, 0, 1), (5, 1, 4), (23, 2, 5), (66, 0, 1), (31, 3, 5)):
        vals, flags, dts, yaw = XM.pair_problem(st, k, i, j, D)
        assert flags.tolist() == [7, 7] and dts[0] == st[4 * D + 1, j, k] - st[4 * D + 1, i, k] and dts[0] > 0
        tr = SM.PolySet(SM.solve_dense(vals, flags, dts, so), SM.yaw_solve(yaw, dts)[:, 0], dts, so, D)
        rows = tr.evaluate(np.array([0.0, tr.T]), TM.WAYPOINT)
        for e, w in enumerate((i, j)):
            assert np.abs(rows[:(so + 1) * D, e] - st[:(so + 1) * D, w, k]).max() <= 1e-12, (k, i, j, e)
            assert abs(rows[4 * D, e] - st[4 * D, w, k]) <= 1e-12
