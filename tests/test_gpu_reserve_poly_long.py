"""mplx_reserve_check_poly (csrc/reserve_poly_kernel.hip) where tests/test_gpu_reserve_poly.py does not go: windows of more
than two blocks of 64 instants, steps at which t_start / step is a rounded quotient, and tables of more than the
kKeep = 4 register tiles in which the partners past them decide.  Inputs: tests/reserve_poly_cases.py (long_hand_case,
long_random_case, inexact_case, keep_case), whose properties tests/test_reserve_poly_long_model.py asserts on the CPU.
As there, the model (tests/reserve_poly_model.py) is fed the table Reservations.positions() returns and the device's own
samples of the problems, and hit, status and n_hit are compared bit for bit; the hand cases also against the hits
written out."""
import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import reserve_poly_cases as RC
import reserve_poly_model as RPM
from test_gpu_reserve_poly import assert_same, load, make_env, make_table, model_of

pytestmark = pytest.mark.gpu


def check(m, D, case, parks, what):
    """The check of the case's candidates against its table, filled per mode of `parks`, against the model; returns
    (got, want) of the first mode."""
    env = make_env(m, D)
    poly = load(env, m, case["cand"])
    out = []
    for park in parks:
        res, rp = make_table(env, m, case, park)
        want = model_of(poly, D, case, res.positions())
        got = res.check_poly(poly, case["t_start"], case["radius"], case["ignore"])
        assert_same(got, want, "%s park=%d" % (what, park))
        out.append((got, want))
        res.free()
        rp.free()
    poly.free()
    env.close()
    return out[0]


@pytest.mark.parametrize("park", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_long_hand_case(engine, D, park):
    """Windows of 128, 129, 153, 192, 193 and 200 instants; a sole conflict in the last lane of a block, the first of the
    next, on both sides of an eight-instant pass, in the third and the fourth block; conflicts in two blocks, in one
    pass, at one instant; a window that ends on the table's last instant; one that began before the clock
    (reserve_poly_cases.LONG_ROWS).  The hits are written out there."""
    case = RC.long_hand_case(D)
    got, _ = check(engine, D, case, [park], "long hand case D=%d" % D)
    assert np.array_equal(got["hit"], case["hit"]), (got["hit"], case["hit"])
    assert not got["status"].any() and got["n_hit"] == len(RC.LONG_ROWS) - 1


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("K", [1, 65])
@pytest.mark.parametrize("D", [2, 3])
def test_long_random_case(engine, D, K, B):
    """random_case at step 1/32 (449 instants): at K = 65 at least a quarter of the problems walk more than two blocks."""
    case = RC.long_random_case(D, K, B)
    got, want = check(engine, D, case, [False, True], "long random D=%d K=%d B=%d" % (D, K, B))
    if K == 65:
        tot = RC.totals(*case["cand"][1:])
        n = np.array([len(RPM.instants(case["step"], case["n_steps"], case["t_start"][k], tot[k])) for k in range(K)])
        print("D=%d K=%d B=%d: %d problems with more than 128 instants, %d hits, %d past the horizon" % (
            D, K, B, (n > 128).sum(), (want[0] >= 0).sum(), (want[0] == -2).sum()))
        assert 4 * (n > 128).sum() >= K and (want[0] == -2).any()
        if B == 65:
            assert 0.2 <= want[2] / float(K) <= 0.8


@pytest.mark.parametrize("robust", [True, False])
def test_long_windows_with_a_lambda(engine, robust):
    """3-D, K = B = 65, the set scaled by scale(2, 0.5): the windows run to the scaled totals, over more than two blocks."""
    m, D, K = engine, 3, 65
    env = make_env(m, D)
    case = RC.long_random_case(D, K, 65, seed=1)
    case["n_steps"] = 8 * 89 + 1
    poly = load(env, m, case["cand"])
    h = poly.scale(2.0, 0.5, robust=robust)
    ok = case["cand"][2] > 0
    assert (h["status"][ok] == 0).all()
    total = poly.info()["total_time"]
    n = np.array([len(RPM.instants(case["step"], case["n_steps"], case["t_start"][k], total[k])) if ok[k] else 0 for k in range(K)])
    res, rp = make_table(env, m, case, False)
    want = model_of(poly, D, case, res.positions())
    print("lambda, robust=%s: %d problems with more than 128 instants (the longest %d), %d hits, %d past the horizon" % (
        robust, (n > 128).sum(), n.max(), (want[0] >= 0).sum(), (want[0] == -2).sum()))
    assert 4 * (n > 128).sum() >= K and (want[0] >= 0).sum() >= 10 and (want[0] == -1).any()
    assert_same(res.check_poly(poly, case["t_start"], case["radius"], case["ignore"]), want, "lambda, robust=%s" % robust)
    for x in (res, rp, poly):
        x.free()
    env.close()


@pytest.mark.parametrize("step", RC.INEXACT_STEPS, ids=["0.1", "1/3"])
@pytest.mark.parametrize("D", [2, 3])
def test_inexact_steps(engine, D, step):
    """Steps 0.1 and 1/3, t_start = fl(i step) and its two neighbours for i up to 5000, one reservation active at the
    single instant i - 1, i or i + 1 (reserve_poly_cases.inexact_case): the first instant of every problem is the one the
    header states, whichever way the quotient t_start / step was rounded.  GONE (the single instants are its)."""
    case = RC.inexact_case(D, step)
    got, _ = check(engine, D, case, [False], "inexact step %r D=%d" % (step, D))
    assert np.array_equal(got["hit"], case["hit"]), (got["hit"], case["hit"])
    assert not got["status"].any() and got["n_hit"] == (case["hit"] >= 0).sum()


@pytest.mark.parametrize("B", [320, 513])
@pytest.mark.parametrize("D", [2, 3])
def test_past_the_register_tiles(engine, D, B):
    """Every reservation a candidate can meet has b >= 256, where the kernel derives exclusion, the ignored group and the
    radius sum anew in every pass; at B = 513 the last tile is one lane."""
    case = RC.keep_case(D, B)
    got, want = check(engine, D, case, [False, True], "past kKeep D=%d B=%d" % (D, B))
    some = want[0] >= 0
    partner = want[0] & 0xffffffff
    print("D=%d B=%d (GONE): %d problems hit a partner >= 256, the largest %d" % (D, B, some.sum(), partner[some].max()))
    assert some.sum() >= 20 and (partner[some] >= 256).all() and (partner[some] == B - 1).any()
