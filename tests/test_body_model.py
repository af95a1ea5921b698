"""CPU: hand cases of tests/body_model.py, the sequential restatement of include/mplx_body.h, the plumbing of the new
header (declared in _abi.py), and the slit scenario of tests/body_cases.py confirmed on the model with the CPU oracle's
successors before any device runs it.  No GPU."""
import math
import os

import numpy as np

import body_cases as BC
import body_model as BM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 9.81


def key(sh, c, a, pts):
    return BM.pair_key(sh, np.asarray(c, dtype=np.float64), np.asarray(a, dtype=np.float64), np.asarray(pts, dtype=np.float64))


def test_upright_disc():
    sh = BM.shape(0.3, 0.1, G)
    assert key(sh, [0, 0, 0], [0, 0, 0], [[0.25, 0, 0]]) == 0          # inside: across the axis, 0.25 < r
    assert key(sh, [0, 0, 0], [0, 0, 0], [[0, 0, 0.25]]) == BM.NO_HIT  # outside: along the axis, 0.25 > h
    # the centre moves with the body
    assert key(sh, [5, -2, 1], [0, 0, 0], [[5.25, -2, 1]]) == 0 and key(sh, [5, -2, 1], [0, 0, 0], [[5, -2, 1.25]]) == BM.NO_HIT
    # the smallest index of several inside; the first is outside
    assert key(sh, [0, 0, 0], [0, 0, 0], [[0, 0, 0.25], [0.1, 0, 0], [0, 0.1, 0]]) == 1


def test_tilted_by_45_degrees_the_offsets_swap_roles():
    """a = (g, 0, 0): the axis is (1, 0, 1) / sqrt 2.  0.25 along the axis is outside (h = 0.1), 0.25 across it inside."""
    sh = BM.shape(0.3, 0.1, G)
    q = 0.25 / math.sqrt(2.0)
    assert key(sh, [0, 0, 0], [G, 0, 0], [[q, 0, q]]) == BM.NO_HIT
    assert key(sh, [0, 0, 0], [G, 0, 0], [[q, 0, -q]]) == 0
    assert key(sh, [0, 0, 0], [G, 0, 0], [[0, 0.25, 0]]) == 0  # the other direction across the axis
    # upright they are the other way round
    assert key(sh, [0, 0, 0], [0, 0, 0], [[q, 0, q]]) == BM.NO_HIT and key(sh, [0, 0, 0], [0, 0, 0], [[q, 0, -q]]) == BM.NO_HIT
    # (upright both lie 0.177 above / below the disc: outside; the pair that swaps is the axis-aligned one)
    assert key(sh, [0, 0, 0], [0, 0, 0], [[0.25, 0, 0]]) == 0 and key(sh, [0, 0, 0], [G, 0, 0], [[0.25, 0, 0]]) == BM.NO_HIT


def test_equal_radii_are_a_sphere():
    rng = np.random.default_rng(1)
    sh = BM.shape(0.4, 0.4, G)
    pts = rng.uniform(-0.6, 0.6, size=(4000, 3))
    dd = (pts ** 2).sum(axis=1)
    clear = np.abs(dd - 0.16) > 1e-12  # (e and dd / r^2 round differently within a few ulp of the surface)
    for a in ([0, 0, 0], [3.0, -7.0, 2.0], [G, G, -G / 2]):
        got = BM.inside(sh, np.zeros(3), np.array(a, dtype=np.float64), pts)
        assert np.array_equal(got[clear], (dd <= 0.16)[clear]) and 0.1 < got.mean() < 0.2  # (the ball fills 0.155 of the cube)


def test_bad_attitudes():
    sh = BM.shape(0.3, 0.1, G)
    pts = [[0.0, 0.0, 0.0]]  # at the centre: inside whenever a point test is made
    assert key(sh, [0, 0, 0], [0, 0, 0], pts) == 0
    assert key(sh, [0, 0, 0], [0, 0, -G], pts) == BM.BAD_ATTITUDE       # thrust vanishes
    assert key(sh, [0, 0, 0], [0, 0, -2 * G], pts) == BM.BAD_ATTITUDE   # thrust points down
    assert key(sh, [0, 0, 0], [0, 0, np.nan], pts) == BM.BAD_ATTITUDE   # a NaN thrust
    # a NaN across the thrust alone fails no comparison of the attitude test as it is written (n_z > 0 holds, and
    # n_z^2 < m^2 nn is false on a NaN): the attitude is not bad, and no point is inside a NaN
    assert key(sh, [0, 0, 0], [np.nan, 0, 0], pts) == BM.NO_HIT
    assert key(BM.shape(0.3, 0.1, G, 0.5), [0, 0, 0], [np.nan, 0, 0], pts) == BM.NO_HIT
    assert key(sh, [0, 0, 0], [1e6, 0, 0], pts) == 0                    # no tilt limit: any thrust that points up
    assert key(sh, [0, 0, 0], [0, 0, -2 * G], np.zeros((0, 3))) == BM.BAD_ATTITUDE  # ... with an empty cloud too


def test_tilt_limit_at_a_representable_boundary():
    """n = (4, 0, 3) with g = 1: n_z^2 = 9 and nn = 25 exactly, and 0.6 * 0.6 * 25 == 9.0 in doubles: AT the limit the test
    n_z^2 < m^2 nn is false (the limit is closed), one ulp above it is true, one ulp below false."""
    a = [4.0, 0.0, 2.0]
    at, above, below = 0.6, float(np.nextafter(0.6, 1.0)), float(np.nextafter(0.6, 0.0))
    assert (at * at) * 25.0 == 9.0 and (above * above) * 25.0 > 9.0 and (below * below) * 25.0 < 9.0
    for m, bad in ((at, False), (above, True), (below, False), (0.0, False), (0.99, True)):
        assert BM.attitude(BM.shape(0.3, 0.1, 1.0, m), a)[2] == bad, m
    # upright passes every limit below 1
    assert not BM.attitude(BM.shape(0.3, 0.1, 1.0, float(np.nextafter(1.0, 0.0))), [0, 0, 5.0])[2]


def test_a_point_on_the_surface_is_inside():
    """r = 0.5, h = 0.25, g = 8: every operand and result below is a dyadic rational, so e == 1.0 exactly."""
    sh = BM.shape(0.5, 0.25, 8.0)
    up = float(np.nextafter(0.5, 1.0))
    assert key(sh, [0, 0, 0], [0, 0, 0], [[0.5, 0, 0]]) == 0 and key(sh, [0, 0, 0], [0, 0, 0], [[up, 0, 0]]) == BM.NO_HIT
    assert key(sh, [0, 0, 0], [0, 0, 0], [[0, -0.5, 0]]) == 0
    top = float(np.nextafter(0.25, 1.0))
    assert key(sh, [0, 0, 0], [0, 0, 0], [[0, 0, 0.25]]) == 0 and key(sh, [0, 0, 0], [0, 0, 0], [[0, 0, top]]) == BM.NO_HIT
    # RR has its slack: the outer conjunct alone admits the point just past r
    assert up * up <= sh["RR"]


def test_two_dimensions_are_the_section_by_the_plane():
    rng = np.random.default_rng(2)
    sh = BM.shape(0.3, 0.12, G, 0.2)
    pts2 = rng.uniform(-0.4, 0.4, size=(3000, 2))
    pts3 = np.concatenate([pts2, np.zeros((3000, 1))], axis=1)
    for _ in range(6):
        c2, a2 = rng.uniform(-0.1, 0.1, size=2), rng.uniform(-12, 12, size=2)
        c3, a3 = np.append(c2, 0.0), np.append(a2, 0.0)
        assert BM.attitude(sh, a2)[2] == BM.attitude(sh, a3)[2]
        if not BM.attitude(sh, a2)[2]:
            got = BM.inside(sh, c2, a2, pts2)
            assert np.array_equal(got, BM.inside(sh, c3, a3, pts3)) and 0 < got.sum() < 3000
        assert key(sh, c2, a2, pts2) == key(sh, c3, a3, pts3)


def test_non_finite_points_never_hit_and_keep_their_index():
    sh = BM.shape(0.3, 0.1, G)
    pts = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [0.1, 0, 0]]
    assert key(sh, [0, 0, 0], [0, 0, 0], pts) == 3


def test_list_check_hand_case():
    """3-D ACC, dt = 1, one parent at rest at the origin, controls +x, +z and -2g z; a point at x = 0.4."""
    sh = BM.shape(0.3, 0.1, G)
    U = np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 0, -2 * G], [0, 0, 0]])
    st = np.zeros((14, 1))
    count, action = np.array([4], np.int32), np.array([0, 1, 2, 7, 0], np.int32)
    cost = np.array([1.0, 1.0, 1.0, 1.0, 1.0])
    out, hit, nb, looked = BM.check(sh, [[0.4, 0, 0]], count, action, cost, 5, [0], st, U, 3, 2, 1.0, 4)
    # +x reaches x = t^2 / 2: 0.125 at sample 2 (t = 0.5), where 0.4 - 0.125 = 0.275 < r (tilted by atan(1 / g), still inside)
    assert looked.tolist() == [True, True, True, False, False]
    assert hit.tolist() == [(2 << 32) | 0, -1, (0 << 32) | BM.BAD_ATTITUDE, -1, -1] and nb == 2
    assert out.tolist() == [np.inf, 1.0, np.inf, 1.0, 1.0]
    assert BM.sample_times(1.0, 4) == [0.0, 0.25, 0.5, 0.75, 1.0]
    # not looked at: a parent_id < 0, a cost that is not finite
    _, hit, nb, looked = BM.check(sh, [[0.4, 0, 0]], count, action, cost, 5, [-1], st, U, 3, 2, 1.0, 4)
    assert not looked.any() and nb == 0 and (hit == -1).all()
    _, hit, nb, looked = BM.check(sh, [[0.4, 0, 0]], count, action, [np.inf, np.nan, 1.0, 1.0, 1.0], 5, [0], st, U, 3, 2, 1.0, 4)
    assert looked.tolist() == [False, False, True, False, False] and nb == 1


def test_poly_times():
    assert BM.poly_times(0.25, 1.0) == [0.0, 0.25, 0.5, 0.75, 1.0, 1.0]  # an exact multiple: the last sample is made twice
    assert BM.poly_times(0.3, 1.0) == [0.0, 0.3, 0.6, np.float64(3) * np.float64(0.3), 1.0]
    assert BM.poly_times(2.0, 1.0) == [0.0, 1.0] and BM.poly_times(0.5, 0.0) == [0.0, 0.0]
    sh = BM.shape(0.3, 0.1, G)
    pos = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    acc = np.zeros((3, 3))
    assert BM.check_poly(sh, [[9.0, 0, 0], [2.2, 0, 0]], 3, pos, acc) == (2 << 32) | 1
    acc[1, 2] = -G
    assert BM.check_poly(sh, [[9.0, 0, 0], [2.2, 0, 0]], 3, pos, acc) == (1 << 32) | BM.BAD_ATTITUDE
    assert BM.check_poly(sh, np.zeros((0, 3)), 3, pos, np.zeros((3, 3))) == BM.NO_HIT


def test_header_and_abi_declare_the_same_symbols(engine):
    from motion_primitive_library_amd import _abi
    src = open(os.path.join(ROOT, "include", "mplx_body.h")).read()
    for name in _abi.BODY_SYMBOLS:
        assert name + "(" in src, name
    assert _abi.BODY_MAX_BYTES == 1 << 30 and "MPLX_BODY_MAX_BYTES = 1 << 30" in src
    assert all(hasattr(engine.search.Body, f) for f in ("fill", "fill_resident", "fill_map", "check", "check_poly",
                                                        "check_poly_resident", "cells", "shape", "free"))


def test_the_slit_on_the_model(engine, oracle_lib):
    """The scenario of tests/body_cases.py on the CPU: the flat body finds the recorded path through the slit, the
    sphere of the same radius finds none."""
    sc = BC.slit(engine)
    flat = BC.slit_model_search(engine, oracle_lib, sc, BC.FLAT)
    print("flat:", flat["out"]["status"], flat["cost"], flat["out"]["rounds"], flat["out"]["expanded"], flat["actions"], flat["stats"])
    assert (flat["out"]["status"], flat["cost"], flat["out"]["rounds"], flat["out"]["expanded"]) == BC.SLIT_FLAT_MODEL[:4]
    assert flat["actions"] == BC.SLIT_FLAT_MODEL[4]
    # the path crosses the wall's plane inside the slit
    xs = flat["states"][0]
    assert xs[0] < sc["wall_x"] < xs[-1]
    ball = BC.slit_model_search(engine, oracle_lib, sc, BC.BALL)
    print("ball:", ball["out"]["status"], ball["out"]["rounds"], ball["out"]["expanded"], ball["stats"])
    assert ball["out"]["status"] == BC.OM.EMPTY and (ball["out"]["rounds"], ball["out"]["expanded"]) == BC.SLIT_BALL_MODEL
