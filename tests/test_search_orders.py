"""No GPU: what the SNP, JRK and yaw cases of the search layer's GPU tests (tests/control_matrix.py) rest on.  The pair
arithmetic of tests/wait_model.py at every control order against the oracle; the numbers the SNP worlds pin, recomputed
from the models on the oracle's lists; and the inputs of the added add_wait cases, which have to feel their acc and
jerk rows on the model alone."""
import itertools

import numpy as np
import pytest

import control_matrix as CM

@pytest.mark.parametrize("dim,control", CM.PAIRS, ids=["%dd-%s" % (d, c.lower()) for d, c in CM.PAIRS])
def test_the_pair_model_is_the_oracle_at_every_order(oracle_lib, dim, control):
    """tests/wait_model.py::pair_eval (successor rows, both lattice hashes, the limits with j_max, the cost) against the
    oracle's dense expansion on a free map, for all 16 pairs: states with live vel, acc and jerk rows, at rest, with a
    jerk inside the hash bin of 0 and one of 1e-20."""
    import wait_model as WM
    O = oracle_lib
    flag = CM.FLAGS[control]
    rng = np.random.default_rng(17 * dim + flag)
    axes = [(-0.5, 0.0, 0.5)] * dim + ([(-0.3, 0.0, 0.3)] if flag & 0x10 else [])
    U = np.array(list(itertools.product(*axes)), dtype=np.float64)
    n, edge = 24, 50
    nodes = np.zeros((4 * dim + 2, n))
    nodes[:dim] = rng.uniform(20.0, 30.0, (dim, n))
    nodes[dim:4 * dim] = np.round(rng.uniform(-1.2, 1.2, (3 * dim, n)), 2)
    nodes[dim:4 * dim, :8] = 0.0
    nodes[3 * dim, 4:8] = [0.04, 1e-20, -0.3, 0.7]
    if flag & 0x10:
        nodes[4 * dim] = rng.uniform(-3.0, 3.0, n)
    nodes[-1] = rng.integers(0, 5, n)
    env = O.Env(dim, flag, U, np.zeros(edge ** dim, np.int8), [edge] * dim, [0.0] * dim, 1.0, dt=1.0, w=10.0, wyaw=0.0,
                v_max=1.0, a_max=1.0, j_max=1.0, yaw_max=0.0)
    d = O.expand(env, nodes)
    seen = set()
    for k in range(n):
        for a in range(len(U)):
            pe = WM.pair_eval(dim, flag, nodes[:, k], U[a], 1.0, 1.0, 1.0, 1.0, 0.0)
            s = k * len(U) + a
            st = int(d["status"][s])
            want = 0 if pe["h_next"] == pe["h_curr"] else 1 if pe["valid"] else 3
            assert st == want, (k, a, st, want)
            assert int(d["hash"][s]) == pe["h_next"], (k, a)
            assert np.array_equal(np.array(pe["next"]).view(np.uint64), d["state"][:, s].view(np.uint64)), (k, a)
            if st == 1:
                assert d["cost"][s] == 0.0 + (pe["J"] + 10.0 * 1.0), (k, a)
            seen.add(st)
    assert seen == ({0, 1, 3} if CM.order_of(flag) >= 2 else {0, 1}), seen


def test_the_numbers_of_the_snp_world_are_the_models(engine, oracle_lib):
    """The (rounds, truncated selections) tests/control_matrix.py pins for the 2D SNP world of tests/test_gpu_open.py, and the
    (rounds, nodes) of the SNP sweeps of tests/test_gpu_table.py: from the models on the oracle's lists, with the conditions
    the world was chosen by (at least three rounds, 100 .. 20 000 nodes, FOUND with closed nodes)."""
    import open_model as OM
    from helpers import oracle_env
    from table_model import TableModel, oracle_provider, sweep
    from test_gpu_open import model_search_on_oracle, small_world_goal
    from test_gpu_parity import _small_world
    from test_table import small_start
    m, O = engine, oracle_lib
    dim, control, g_max, edge = CM.SNP_WORLD
    wl, start, h0, goal = small_world_goal(m, O, dim, control, g_max, edge)
    assert start[2 * dim] != 0 and start[3 * dim + 1] != 0  # live acc and jerk rows
    for (eps, delta, cap), want in CM.SNP_WORLD_ROUNDS.items():
        status, rounds, truncated, closed, reopened, nodes = model_search_on_oracle(O, wl, dim, control, start, h0, goal, eps, delta, cap,
                                                                                    g_max, 10.0, wl.params["v_max"])
        assert status == OM.FOUND and (rounds, truncated) == want and rounds >= 3 and closed >= 1 and 100 <= nodes <= 20000
    for name, dim, control, g_max, max_rounds, edge in CM.SWEEP_ADDED:
        wl = _small_world(m, dim, control, seed=5, edge=edge)
        start = np.array(CM.live_start(small_start(wl), dim, control))
        t = TableModel(4 * dim + 2)
        rounds, _ = sweep(t, oracle_provider(O, oracle_env(wl)), start, [O.lattice_hash(dim, control, start)], g_max=g_max,
                          max_rounds=max_rounds)
        assert rounds >= 3 and 100 < t.n_nodes <= 20000, (name, rounds, t.n_nodes)
        if CM.SWEEP_MODEL[name] is not None:
            assert (rounds, t.n_nodes) == CM.SWEEP_MODEL[name], name
        else:
            assert control & CM.YAW and rounds == 4


@pytest.mark.parametrize("case", CM.WAIT_ADDED, ids=[CM.wait_id(*c) for c in CM.WAIT_ADDED])
def test_the_wait_inputs_feel_their_acc_and_jerk_rows(engine, case):
    """The sensitivity check of tests/test_gpu_wait.py on the model alone, and the shares the GPU test asserts of it."""
    import test_gpu_wait as TW
    import wait_model as WM
    dim, control, yaw, nU, S = case
    U, flag, order, F, goal, pst, kind, count, parent_id, a0 = TW.wait_case(engine, dim, control, CM.THREE, yaw, nU, S)
    if order >= 3:
        moved = TW.assert_wait_case_is_sensitive(dim, control, yaw, nU, S, U, flag, order, F, goal, pst, kind, count, parent_id)
        assert sorted(moved) == (["acc", "jrk"] if order == 4 else ["acc"])
    host = {"stride": S, "count": count.copy(), "action": np.zeros(TW.N_ALLOC * S, np.int32), "cost": np.zeros(TW.N_ALLOC * S)}
    n_added, eligible = WM.add_wait(host, TW.N_ROWS, pst, parent_id, dim, flag, U, 1.0, 10.0, 3.0, 3.0, 0.0, 0.5 if yaw else 0.0, goal)
    assert 0.2 <= n_added / TW.N_ROWS <= 0.8
    if order >= 2:
        assert eligible[kind == 0].all() and eligible[kind == 3].all() and not eligible[kind == 1].any() and not eligible[kind == 2].any()
        assert 0.2 <= eligible.mean() <= 0.8
    else:
        assert eligible.all()
    if order >= 4:
        assert (np.abs(pst[3 * dim:4 * dim, :TW.N_ROWS]).max(axis=0)[kind == 1] > 0).sum() >= 3  # movers with a jerk
