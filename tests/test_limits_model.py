"""tests/limits_model.py against exact arithmetic, and its quirks pinned bit for bit (no GPU).

Model sanity: on 400 seeded JRK two-point quintics the model's max_vel / max_acc / max_jrk stay within 2 * 2^-52 * scale
of the truth (limits_model.truth_reference / truth_all; scale = the sum of the absolute terms of the polynomial at T).
The run that prepared this test gave 0.46 (vel), 0.66 (acc), 0.48 (jrk) in both modes; the factor over that is room
for another seed's tail -- a draw that exceeds it is a model bug to find, not a constant to raise.

The quirks: crafted coefficients with dyadic roots, so every expected value below is exact arithmetic done by hand.

Two notes on cases one might expect here:
  * an acos argument ABOVE 1 cannot be reached in float64: the acos branch needs fl(Q^3 + R^2) < 0, i.e. fl(R^2) < w =
    fl(-Q^3) (the sum of two nearby numbers of opposite sign is exact), while an argument above 1 needs |R| > fl(sqrt(w))
    with a correctly rounded sqrt, which gives fl(R^2) >= w.  What can be reached is an argument of exactly 1 with a
    negative discriminant; that case is pinned (ACOS_ONE).  The clamp of ALL_ROOTS only matters where sqrt is not
    correctly rounded.
  * the reference's extrema_j returns -c1 * 2 / c0, twice the time at which the jerk's derivative vanishes; REFERENCE
    keeps it, ALL_ROOTS adds the true extremum (JERK_PARABOLA)."""
import numpy as np
import pytest

import limits_model as LM

REF, ALL = LM.REFERENCE, LM.ALL_ROOTS
EPS = 2.0 ** -52
JRK, ACC, VEL, SNP = 0x07, 0x03, 0x01, 0x0F


def same(x, want):
    return np.float64(x).view(np.uint64) == np.float64(want).view(np.uint64)


@pytest.mark.parametrize("mode", [REF, ALL], ids=["reference", "all_roots"])
def test_model_against_truth(mode):
    ref = LM.quintic_reference()
    assert len(ref) == LM.N_QUINTICS
    for order in (1, 2, 3):
        worst = 0.0
        for n, row in enumerate(ref):
            r = row[(mode, order)]
            assert not r["near"], (n, order)  # no root within 2^-30 T of an end: nothing is left out, here or on the device
            ratio = r["e_ref"] / (EPS * r["scale"])
            worst = max(worst, ratio)
            assert ratio <= 2.0, "quintic %d, order %d: |model - truth| = %.3g = %.2f * 2^-52 * scale" % (n, order, r["e_ref"], ratio)
        print("mode %d order %d: worst |model - truth| / (2^-52 scale) = %.3f" % (mode, order, worst))


def test_hidden_roots_exist():
    """On at least a quarter of the quintics the reference's max_vel misses a root inside (0, T) that ALL_ROOTS sees:
    the two modes are not the same function."""
    ref = LM.quintic_reference()
    hidden = sum(row[(ALL, 1)]["model"] > row[(REF, 1)]["model"] for row in ref)
    print("hidden velocity roots on %d of %d quintics" % (hidden, len(ref)))
    assert hidden >= len(ref) // 4
    assert all(row[(ALL, o)]["model"] >= row[(REF, o)]["model"] for row in ref for o in (1, 2, 3))


# (name, c(0) .. c(5), T, order, REFERENCE, ALL_ROOTS)
HIDDEN_QUAD_V = ("a = -3 (t - 1)(t - 3), b < 0: quad returns 3 first, 3 >= T ends the scan, the root 1 is never seen",
                 [0, -6, 12, -9, 0, 0], 2.0, 1, 2.0, 4.0)                      # v = -t^3 + 6 t^2 - 9 t: v(1) = -4, v(2) = -2
HIDDEN_QUAD_A = ("j = -3 (t - 1)(t - 3) through extrema_a's quad", [-6, 12, -9, 0, 0, 0], 2.0, 2, 2.0, 4.0)
NO_REAL_ROOT = ("p < 0: a = -3 t^2 - 3 never vanishes", [0, -6, 0, -3, 0.5, 0], 1.0, 1, 3.5, 3.5)     # v(1) = -1 - 3 + 0.5
NAN_QUAD = ("c c and 4 b d overflow: p = inf - inf = NaN is not < 0, both roots are NaN and are passed over",
            [0, 2e200, 1e200, 1e200, 0, 0], 1.0, 1, float.fromhex("0x1.3292c1b301a28p+665"), float.fromhex("0x1.3292c1b301a28p+665"))
NAN_CUBIC = ("c1 = 0 and a denormal c0 != 0: the cubic is entered, a0 = inf, R - sqrt(D) = inf - inf: a NaN root",
             [1e-320, 0, 0, 1.0, 0, 0], 1.0, 1, 1.0, 1.0)
TRIPLE_ROOT = ("a = (t - 1)^3: Q = R = D = 0 exactly, the roots 1 and 1", [6, -6, 3, -1, 0, 0], 2.0, 1, 0.25, 0.25)  # v(1) = -1/4
ACOS_ONE = ("D < 0 and R / sqrt(-Q^3) == 1 exactly: theta = 0, the largest root 2.5633.. first, the double root negative",
            [6.0, 0.0, -4.928, -4.210698662041551, 0.25, 0.0], 3.0, 1, float.fromhex("0x1.fe157c2171f8ep+3"),
            float.fromhex("0x1.fe157c2171f8ep+3"))
NO_JERK_ROOT = ("c0 == 0: extrema_j is empty, j = 3 t - 2", [0, 3, -2, 0, 0, 0], 1.5, 3, 2.5, 2.5)
JERK_PARABOLA = ("j = 2 t^2 - 8 t + 1: the reference looks at t = 4 >= T, the extremum is at 2: j(2) = -7, j(3) = -5",
                 [4, -8, 1, 0, 0, 0], 3.0, 3, 5.0, 7.0)
JERK_INSIDE = ("j = 2 t^2 - 3 t + 1: the reference's 1.5 is inside and no extremum: j(1.5) = 1, j(2) = 3", [4, -3, 1, 0, 0, 0], 2.0, 3, 3.0, 3.0)
LINEAR = ("a = 2 t - 1 through solve's linear branch: v = t^2 - t + 0.125, v(0.5) = -0.125, v(2) = 2.125", [0, 0, 2, -1, 0.125, 0], 2.0, 1, 2.125, 2.125)
CASES = [HIDDEN_QUAD_V, HIDDEN_QUAD_A, NO_REAL_ROOT, NAN_QUAD, NAN_CUBIC, TRIPLE_ROOT, ACOS_ONE, NO_JERK_ROOT, JERK_PARABOLA,
         JERK_INSIDE, LINEAR]
# the ones whose result does not pass through cbrt / acos / cos with a finite argument: bit for bit on any device
IEEE_ONLY = [HIDDEN_QUAD_V, HIDDEN_QUAD_A, NO_REAL_ROOT, NAN_QUAD, NAN_CUBIC, NO_JERK_ROOT, JERK_PARABOLA, JERK_INSIDE, LINEAR]


@pytest.mark.parametrize("case", CASES, ids=[c[0].split(":")[0][:40] for c in CASES])
def test_quirks_bit_for_bit(case):
    _, c, T, order, want_ref, want_all = case
    assert same(LM.axis_max(c, T, order, REF), want_ref), (LM.axis_max(c, T, order, REF), want_ref)
    assert same(LM.axis_max(c, T, order, ALL), want_all), (LM.axis_max(c, T, order, ALL), want_all)


def test_quirk_roots():
    """The roots behind the cases above, as solve returns them."""
    assert LM.extrema(HIDDEN_QUAD_V[1], 1, REF) == [3.0, 1.0]      # the larger root first
    assert LM.extrema(HIDDEN_QUAD_A[1], 2, REF) == [3.0, 1.0]
    assert LM.extrema(NO_REAL_ROOT[1], 1, REF) == []
    assert all(np.isnan(r) for r in LM.extrema(NAN_QUAD[1], 1, REF)) and len(LM.extrema(NAN_QUAD[1], 1, REF)) == 2
    assert all(np.isnan(r) for r in LM.extrema(NAN_CUBIC[1], 1, ALL)) and len(LM.extrema(NAN_CUBIC[1], 1, ALL)) == 1
    assert LM.extrema(TRIPLE_ROOT[1], 1, REF) == [1.0, 1.0]
    r = LM.extrema(ACOS_ONE[1], 1, REF)
    assert len(r) == 3 and r[0] > 2.5 and r[1] < 0 and r[2] < 0 and not np.isnan(r).any()
    assert [float(x).hex() for x in r] == [float(x).hex() for x in LM.extrema(ACOS_ONE[1], 1, ALL)]  # the clamp changes nothing
    assert LM.extrema(JERK_PARABOLA[1], 3, REF) == [4.0] and LM.extrema(JERK_PARABOLA[1], 3, ALL) == [4.0, 2.0]
    assert LM.extrema(LINEAR[1], 1, REF) == [0.5]
    # in the acos branch the first root is the largest one
    coef, Ts = LM.quintics()
    three = [LM.extrema(c, 1, REF) for c in coef]
    three = [r for r in three if len(r) == 3]
    assert len(three) > 100 and all(r[0] >= r[1] and r[0] >= r[2] for r in three)


def test_limits_and_controls():
    """validate_primitive per control, a limit <= 0, a limit exactly at the maximum (valid: the comparison is >), the
    first bad segment, and the exceed bits, on a two-segment 2-D trajectory built from the cases above."""
    seg0 = [np.array(LINEAR[1], float), np.zeros(6)]  # axis 0: vel 2.125, acc max(|-1|, |3|) = 3, jrk 2
    seg1 = [np.array(JERK_PARABOLA[1], float), np.array(NO_JERK_ROOT[1], float)]
    coefs, dts = [seg0, seg1], [2.0, 3.0]
    free = LM.traj_limits(coefs, dts, SNP, 0.0, -1.0, 0.0, REF)
    assert free["valid"] == 1 and free["first_bad"] == -1 and free["exceed"] == 0
    mv, ma, mj = (float(free[k].max()) for k in ("max_vel", "max_acc", "max_jrk"))
    assert free["max_vel"][0] >= 2.125 and free["max_acc"][0] >= 3.0
    at = LM.traj_limits(coefs, dts, SNP, mv, ma, mj, REF)
    assert at["valid"] == 1 and at["exceed"] == 0                     # exactly at the maxima: >, not >=
    below = np.nextafter
    for control, expect in ((VEL, (1, 1, 1)), (ACC, (0, 1, 1)), (JRK, (0, 0, 1)), (SNP, (0, 0, 0)), (0x17, (0, 0, 1))):
        for q, (key, bit) in enumerate((("max_vel", 1), ("max_acc", 2), ("max_jrk", 4))):
            lim = [mv, ma, mj]
            lim[q] = float(below(lim[q], 0.0))
            r = LM.traj_limits(coefs, dts, control, *lim, REF)
            assert r["exceed"] == bit, (control, key)                  # exceed does not depend on the control
            assert r["valid"] == expect[q], (control, key)
            if not expect[q]:
                per_seg = [max(float(LM.axis_max(cs[i], t, q + 1, REF)) for i in range(2)) for cs, t in zip(coefs, dts)]
                assert r["first_bad"] == int(np.argmax(np.array(per_seg) > lim[q]))
            else:
                assert r["first_bad"] == -1
    # both segments bad: the first one is reported
    r = LM.traj_limits(coefs, dts, ACC, 0.1, 0.0, 0.0, REF)
    assert r["valid"] == 0 and r["first_bad"] == 0 and r["exceed"] == 1
    # the modes differ on the jerk of segment 1
    assert LM.traj_limits(coefs, dts, SNP, 0, 0, 0, ALL)["max_jrk"][0] == 7.0 and free["max_jrk"][0] == 5.0
