"""tests/reserve_poly_model.py (the sequential restatement of include/mplx_reserve_poly.h) against a brute force over
every (instant, reservation), against tests/conflict_model.py on one merged set, and the timed admission rule through
the dynamic programme of tests/shortcut_model.py.  No GPU: positions come from tests/reserve_poly_cases.py."""
import numpy as np
import pytest

import conflict_model as CM
import reserve_poly_cases as RC
import reserve_poly_model as RPM
import shortcut_model as SHM


def model_inputs(case, park=False):
    c, dts, n_segs = case["cand"]
    rc, rd, rs = case["res"]
    table = RC.host_table(rc, rd, rs, case["step"], case["n_steps"], case["t0"], case["r_b"], case["group"], park)
    status = np.where(n_segs == 0, 1, 0).astype(np.uint8)  # SOLVE_EMPTY
    return status, n_segs, RC.totals(dts, n_segs), table, lambda k, i, tl: RC.segs_position(c, dts, n_segs, k, tl)


def run(case, park=False, brute=False):
    status, n_segs, total, table, own = model_inputs(case, park)
    return RPM.check(status, n_segs, total, case["t_start"], case["radius"], case["ignore"], case["step"], table, own, brute=brute)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("K,B", [(1, 1), (9, 0), (33, 17), (65, 65)])
def test_model_against_brute_force(D, K, B):
    case = RC.random_case(D, K, B)
    for park in (False, True):
        hit, status, n_hit = run(case, park)
        hit_b, status_b, n_hit_b = run(case, park, brute=True)
        assert np.array_equal(hit, hit_b) and np.array_equal(status, status_b) and n_hit == n_hit_b
        assert n_hit == int((hit != -1).sum())
        if B == 0:
            assert ((hit == -1) | (hit == -2)).all()


@pytest.mark.parametrize("D", [2, 3])
def test_the_random_case_is_not_vacuous(D):
    """The case the GPU test compares bit for bit: between 20 % and 80 % of the problems have a hit, at least one leaves
    the horizon, hits at the first instant of a problem and later ones are both present."""
    case = RC.random_case(D, 65, 65)
    hit, _, n_hit = run(case)
    share = n_hit / 65.0
    print("D=%d: share of problems with a hit %.3f, %d past the horizon" % (D, share, (hit == -2).sum()))
    assert 0.2 <= share <= 0.8, share
    assert (hit == -2).any() and (hit == -1).any() and (hit >= 0).any()
    first = [RPM.instants(case["step"], case["n_steps"], case["t_start"][k], RC.totals(*case["cand"][1:])[k]) for k in range(65)]
    later = [k for k in range(65) if hit[k] >= 0 and (hit[k] >> 32) > first[k][0]]
    assert later, "no hit later than a problem's first instant"


@pytest.mark.parametrize("park", [False, True])
def test_hand_case(park):
    case = RC.hand_case(park)
    hit, status, n_hit = run(case, park)
    assert np.array_equal(hit, case["hit"]), (hit, case["hit"])
    assert np.array_equal(status, case["status"])
    assert n_hit == int((case["hit"] != -1).sum())


def test_the_scan_finds_the_stated_instants():
    rng = np.random.default_rng(77)
    for _ in range(2000):
        step = float(rng.choice([0.25, 0.1, 0.3, 1.0 / 3.0, 0.7]))
        n_steps = int(rng.integers(1, 90))
        ts = float(rng.choice([rng.uniform(-5, 25), rng.integers(-20, 100) * step, rng.integers(-8, 40) / 4.0]))
        total = float(rng.choice([rng.uniform(0, 20), rng.integers(0, 60) * step, 0.0]))
        if RPM.leaves_horizon(step, n_steps, ts, total):
            continue
        assert np.array_equal(RPM.instants(step, n_steps, ts, total), RPM.instants_scan(step, n_steps, ts, total)), (step, n_steps, ts, total)


@pytest.mark.parametrize("D", [2, 3])
def test_composition_with_the_conflict_model(D):
    """Candidates and reservations in ONE set under MPLX_CONFLICT_GONE: hit[k] = min over the reserved b of
    (pair_first[k][b] << 32 | b).  Candidates that leave the horizon are compared on a table long enough to hold them
    (the merged set knows no horizon); candidates get a group of their own each, reservations theirs, nobody ignores."""
    K, B = 33, 17
    case = RC.random_case(D, K, B)
    case["n_steps"] = 120
    case["ignore"] = np.full(K, -1, np.int32)
    status, n_segs, total, table, own = model_inputs(case, park=False)
    hit, _, _ = RPM.check(status, n_segs, total, case["t_start"], case["radius"], None, case["step"], table, own)
    assert not (hit == -2).any() and (hit >= 0).any() and (hit == -1).any()
    # the merged set: candidates first
    c, dts, ns = case["cand"]
    rc, rd, rs = case["res"]
    mc, md, mn = np.concatenate([c, rc], axis=3), np.concatenate([dts, rd], axis=1), np.concatenate([ns, rs])
    t0 = np.concatenate([case["t_start"], case["t0"]])
    rad = np.concatenate([case["radius"], case["r_b"]])
    group = np.concatenate([1000 + np.arange(K), case["group"]])
    merged = RC.host_table(mc, md, mn, case["step"], case["n_steps"], t0, rad, group, park=False)
    pos = np.ascontiguousarray(merged["pos"].transpose(0, 2, 1))
    res = CM.conflicts(pos, merged["active"] != 0, rad, merged["included"] != 0, group=group)
    want = RPM.from_pair_first(res["pair_first"], range(K), range(K, K + B))
    assert np.array_equal(hit, want), (hit, want)


def test_timed_admission_in_the_programme():
    """shortcut_model.dp on the masked cost matrix: never cheaper than the untimed programme, equal to it (cost and kept
    states) where no non-adjacent edge has a hit, and the adjacent chain is always admitted."""
    rng = np.random.default_rng(5)
    some_dearer = 0
    for trial in range(200):
        W = int(rng.integers(2, 12))
        hop = int(rng.integers(1, W))
        c = rng.uniform(0.5, 3.0, (W - 1, hop)) * (1 + np.arange(hop))[None, :] * 0.6
        c[rng.random((W - 1, hop)) < 0.2] = np.inf
        c[:, 0] = rng.uniform(0.5, 3.0, W - 1)
        for i in range(W - 1):
            c[i, W - 1 - i:] = np.inf  # past the chain
        hit = np.where(rng.random((W - 1, hop)) < (0.0 if trial % 4 == 0 else 0.3), rng.integers(0, 1 << 40, (W - 1, hop)), -1)
        hit[rng.random((W - 1, hop)) < 0.05] = -2
        free = SHM.dp(c, W, hop)
        timed = SHM.dp(RPM.admit(c, hit), W, hop)
        assert timed[0] == 0 and np.isfinite(timed[2]) and timed[2] >= free[2]
        if (hit[:, 1:] == -1).all():
            assert timed[2] == free[2] and list(timed[1]) == list(free[1])
        some_dearer += timed[2] > free[2]
        only_chain = SHM.dp(RPM.admit(c, np.full((W - 1, hop), 5)), W, hop)
        assert list(only_chain[1]) == list(range(W))
        assert RPM.chain_hit(np.full((W - 1, hop), -1), W) == -1
    assert some_dearer > 20
    assert RPM.chain_hit(np.array([[-1, 3], [7, -1], [5, -1], [2, -1]]), 4) == 5
    assert RPM.chain_hit(np.array([[-1, 3], [-2, -1]]), 3) == -2


@pytest.mark.parametrize("so", [0, 1, 2])
@pytest.mark.parametrize("D", [2, 3])
def test_a_rest_pair_solves_to_the_constant(D, so):
    """A wait edge leaves a repeated state with t_{i+1} > t_i; its pair is p -> p with zero derivatives over dt > 0.
    solve_model.solve_block, the twin of the pair solve, gives status 0 (not None) and EXACTLY the constant: p_0 = p,
    every other coefficient zero -- so the shortcuts need no special case for rest pairs (include/mplx_reserve_poly.h)."""
    import solve_model as SM
    rng = np.random.default_rng(31 + 10 * D + so)
    for dt in [0.1, 0.25, 0.3, 0.5, 1.0, 1.0 / 3.0, 2.5, 8.0, 80.0] + list(rng.uniform(0.05, 20.0, 40)):
        p = rng.uniform(-50.0, 50.0, D)
        vals = np.zeros((3, 2, D))
        vals[0, 0] = vals[0, 1] = p
        c = SM.solve_block(vals, np.array([7, 7], np.uint8), np.array([dt]), so)
        assert c is not None and np.array_equal(c[0], p) and (c[1:] == 0.0).all(), (dt, p, c)
