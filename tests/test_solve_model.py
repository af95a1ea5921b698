"""CPU: the two models of the trajectory solver (tests/solve_model.py; include/mplx_solve.h) against each other and against
the statement of the problem, and the ctypes structs against the header.  No GPU.

solve_dense (poly_solver.cpp restated in float64) is held to solve_exact (the same statement in exact rationals) by a
bound that comes from the problem, not from either model: an LU solve of a system of order n loses at most about
n * eps * cond relative to its solution, and the dense solve chains two of them -- the free system Rpp and the
segment's own N x N block of A -- so |dense - exact| <= (n_free * cond_2(Rpp) + N * max_s cond_2(A_s)) * 2^-52 * scale,
with a floor of 64 * 2^-52 * scale (a handful of roundings per coefficient); scale is the largest exact coefficient.

solve_block, the float64 twin of csrc/solve_kernel.hip's own elimination, is held to solve_exact by the bound the device
is held to (tests/test_gpu_solve.py): e <= 8 * max(e_ref, 2^-52 * scale) with e_ref the error of solve_dense; at
smoothing order 0 it is solve_dense bit for bit.  The worst ratios are printed (pytest -s)."""
import ctypes as C
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import solve_model as SM
from test_table import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
CASES = SM.cpu_cases()
IDS = [c[0] for c in CASES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("so", [0, 1, 2])
def test_dense_is_exact_to_rounding(case, so):
    name, vals, dts = case
    flags = SM.path_flags(vals.shape[1], so)
    exact = SM.solve_exact(vals, flags, dts, so)
    dense = SM.solve_dense(vals, flags, dts, so)
    R, ids, fixed = SM.exact_setup(vals, flags, dts, so)
    free = [i for i, f in enumerate(fixed) if not f]
    cond = np.linalg.cond(np.array([[float(R[i][j]) for j in free] for i in free])) if free else 1.0
    N = 2 * (so + 1)
    A = np.array(SM._system(vals.shape[1], dts, so, flags, np.float64)[0], dtype=np.float64)
    cond_a = max(np.linalg.cond(A[i * N:(i + 1) * N, i * N:(i + 1) * N]) for i in range(vals.shape[1] - 1))
    scale = SM.scale_of(exact)
    err = SM.max_err(dense, exact)
    bound = max((len(free) * cond + N * cond_a) * EPS, 64 * EPS) * scale
    print("%s so=%d: |dense - exact| / scale = %.3g, bound / scale = %.3g (cond %.3g)" % (name, so, err / scale, bound / scale, cond))
    assert err <= bound


@pytest.mark.parametrize("case", CASES, ids=IDS)
@pytest.mark.parametrize("so", [0, 1, 2])
def test_exact_solution_is_continuous_and_meets_the_fixed_values(case, so):
    name, vals, dts = case
    W, D, h = vals.shape[1], vals.shape[2], so + 1
    flags = SM.path_flags(W, so)
    d0, dT = SM.derivs_of(SM.solve_exact(vals, flags, dts, so), dts, so)
    for s in range(W - 2):  # every derivative below so + 1 is continuous at the interior waypoints
        assert dT[s] == d0[s + 1], (name, s)
    for w in range(W):
        for k in range(h):
            if flags[w] & (1 << k):
                want = [Fraction(float(vals[k][w][i])) for i in range(D)]
                if w < W - 1:
                    assert d0[w][k] == want, (name, w, k)
                if w > 0:
                    assert dT[w - 1][k] == want, (name, w, k)


@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[4]], ids=[IDS[0], IDS[2], IDS[4]])
@pytest.mark.parametrize("so", [1, 2])
def test_exact_solution_is_the_minimum(case, so):
    """Perturbing any free derivative by +-1e-3 raises the exact cost."""
    name, vals, dts = case
    W, D, h = vals.shape[1], vals.shape[2], so + 1
    flags = SM.path_flags(W, so)
    p, cost = SM.solve_exact(vals, flags, dts, so, want_cost=True)
    R, ids, fixed = SM.exact_setup(vals, flags, dts, so)
    d0, dT = SM.derivs_of(p, dts, so)
    x = [d0[w][k] if w < W - 1 else dT[w - 1][k] for (w, k) in ids]
    assert SM.exact_cost(x, R) == cost
    n_free = 0
    for i, f in enumerate(fixed):
        if f:
            continue
        n_free += 1
        for a in range(D):
            for step in (Fraction(1, 1000), Fraction(-1, 1000)):
                y = [list(row) for row in x]
                y[i][a] += step
                assert SM.exact_cost(y, R) > cost, (name, ids[i], a)
    assert n_free == (W - 2) * so


def test_smoothing_order_zero_is_the_closed_form_bit_for_bit():
    """so = 0: nothing is free, p0 = pos_w and p1 = (pos_{w+1} - pos_w) / T (the 2 x 2 LU's pivots tie and do not swap);
    the yaw solve likewise."""
    for name, vals, dts in CASES:
        W = vals.shape[1]
        p = SM.solve_dense(vals, SM.path_flags(W, 0), dts, 0)
        for s in range(W - 1):
            assert np.array_equal(bits(p[2 * s]), bits(vals[0][s])), (name, s)
            assert np.array_equal(bits(p[2 * s + 1]), bits((vals[0][s + 1] - vals[0][s]) / np.float64(dts[s]))), (name, s)
        yaw = np.linspace(-1.0, 2.0, W) * 1.1
        py = SM.yaw_solve(yaw, dts)
        for s in range(W - 1):
            assert bits(py[2 * s])[0] == bits(yaw[s])[0] and bits(py[2 * s + 1])[0] == bits((yaw[s + 1] - yaw[s]) / np.float64(dts[s]))[0]


def test_time_allocation_and_primitives():
    dts = SM.allocate_time(SM.REF_PATH, 1.0)
    assert dts.tolist() == [1.0, 1.0, 3.0] and SM.set_time(dts).tolist() == [0.0, 1.0, 2.0, 5.0]
    assert SM.allocate_time(SM.REF_PATH, 0.0).size == 0 and SM.allocate_time(SM.REF_PATH[:1], 1.0).size == 0
    p = SM.solve_dense(SM.path_vals(SM.REF_PATH), SM.path_flags(4, 2), dts, 2)
    ps = SM.PolySet(p, SM.yaw_solve(np.zeros(4), dts)[:, 0], dts, 2, 2)
    c = SM.to_primitive_coeffs(p, 2)
    assert np.array_equal(c[1, 0], [p[11, 0] * 120, p[10, 0] * 24, p[9, 0] * 6, p[8, 0] * 2, p[7, 0], p[6, 0]])
    rows = ps.evaluate(ps.taus, SM.tm.WAYPOINT)  # at its taus the trajectory is at its waypoints, to rounding
    assert np.allclose(rows[:2].T, SM.REF_PATH, rtol=0, atol=1e-12)
    assert ps.T == 5.0 and ps.effort[2] > 0.0


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_solve.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_structs_and_symbols_match_the_header(engine):
    """Size and every field offset of the ctypes structs, checked by the C compiler against include/mplx_solve.h."""
    A = engine._abi
    syms = _declared("mplx_solve.h")
    assert sorted(A.SOLVE_SYMBOLS) == syms and len(syms) == 10
    lib = A.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s
    src = ["#include <stddef.h>", '#include "mplx_solve.h"']
    for cname, st in (("mplx_solve_in", A.SolveIn), ("mplx_solve_out", A.SolveOut)):
        src.append("_Static_assert(sizeof(%s) == %d, \"size of %s\");" % (cname, C.sizeof(st), cname))
        for f, _ in st._fields_:
            src.append("_Static_assert(offsetof(%s, %s) == %d, \"%s.%s\");" % (cname, f, getattr(st, f).offset, cname, f))
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c11", "-I", os.path.join(ROOT, "include"), "-"],
                       input="\n".join(src) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (A.SOLVE_EMPTY, A.SOLVE_BAD_TIME, A.SOLVE_SINGULAR) == (1, 2, 8) and (A.USE_POS, A.USE_VEL, A.USE_ACC) == (1, 2, 4)
    assert lib.mplx_abi_version() == 9  # unchanged
    # the entry points check their arguments before they touch a device
    assert lib.mplx_poly_create(None, 1, 2, None) == A.ERR_ARG
    assert lib.mplx_solve_device(None, None, None) == A.ERR_ARG and lib.mplx_solve(None, None, None) == A.ERR_ARG
    assert lib.mplx_poly_info(None, None) == A.ERR_ARG and lib.mplx_poly_sample(None, None, None) == A.ERR_ARG
    assert lib.mplx_poly_traverse(None, 0, None) == A.ERR_ARG
    for name in ("solve_traj", "solve_traj_resident", "alloc_poly"):
        assert hasattr(engine.EnvMap, name)
    assert hasattr(engine.search.SearchResult, "smooth") and hasattr(engine.search.MultiSearchResult, "smooth")
    for name in ("setPath", "setWaypoints", "setV", "setDts", "solve", "getDts", "getWaypoints"):
        assert hasattr(engine.TrajSolver, name)


# ------------------------------------------------------------------------------------- the twin of the kernel, solve_block
FACTOR = 8.0  # the project's bound: e <= 8 * max(e_ref, 2^-52 * scale), tests/test_gpu_solve.py


def block_ratio(vals, flags, dts, so, what):
    """e_blk / max(e_ref, 2^-52 scale) of solve_block against solve_exact, e_ref that of solve_dense; asserts <= FACTOR."""
    exact = SM.solve_exact(vals, flags, dts, so)
    scale = SM.scale_of(exact)
    e_ref, e_blk = SM.max_err(SM.solve_dense(vals, flags, dts, so), exact), SM.max_err(SM.solve_block(vals, flags, dts, so), exact)
    floor = max(e_ref, EPS * scale)
    assert e_blk <= FACTOR * floor, "%s: e_blk %.3g, e_ref %.3g, scale %.3g: ratio %.2f" % (what, e_blk, e_ref, scale, e_blk / floor)
    return e_blk / floor


@pytest.mark.parametrize("so", [0, 1, 2])
def test_block_twin_on_the_cpu_cases(so):
    worst = 0.0
    for name, vals, dts in CASES:
        worst = max(worst, block_ratio(vals, SM.path_flags(vals.shape[1], so), dts, so, name))
    print("solve_block, cpu cases, so = %d: worst ratio %.3f" % (so, worst))


@pytest.mark.parametrize("D,so", [(D, so) for D in (2, 3) for so in (1, 2)], ids=lambda x: str(x))
def test_block_twin_on_the_k67_sets(D, so):
    """The K = 67, w_max = 7 sets of tests/test_gpu_solve.py (given durations)."""
    from test_gpu_solve import problems, vals_of, w_of
    wp, _, dts, _ = problems(D)
    worst = 0.0
    for k in range(wp.shape[2]):
        W = w_of(k)
        if W >= 2:
            worst = max(worst, block_ratio(vals_of(wp, k, W, D), SM.path_flags(W, so), dts[:W - 1, k], so, "problem %d" % k))
    print("solve_block, K = 67 set, D = %d, so = %d: worst ratio %.3f" % (D, so, worst))


@pytest.mark.parametrize("D,so", [(D, so) for D in (2, 3) for so in (1, 2)], ids=lambda x: str(x))
def test_block_twin_on_the_exact_subset_of_the_long_set(D, so):
    """solve_model.LONG_EXACT: the problems tests/test_gpu_poly_long.py holds to solve_exact on the device (W <= 24, every
    duration pattern).  The seed of the long set was chosen with these ratios, all below FACTOR, before any device run."""
    wp = SM.long_problems(D)[0]
    for mode, ks in SM.LONG_EXACT.items():
        worst = 0.0
        for k in ks:
            W = SM.long_w(k)
            worst = max(worst, block_ratio(SM.long_vals(wp, k, W, D), SM.path_flags(W, so), SM.long_durations(D, mode, k), so,
                                           "problem %d (W = %d, %s, %s)" % (k, W, SM.long_pattern(k), mode)))
        print("solve_block, long set, D = %d, so = %d, %s: worst ratio %.3f" % (D, so, mode, worst))


@pytest.mark.parametrize("D", [2, 3])
def test_block_twin_is_the_dense_model_bit_for_bit_at_order_zero(D):
    """so = 0 at every W and every duration pattern of the long set, given and allocated durations."""
    wp = SM.long_problems(D)[0]
    seen = set()
    for k in range(3 * len(SM.LONG_NWP)):  # the first three problems of every W class: random, alternating, geometric
        W = SM.long_w(k)
        for mode in ("given", "alloc_arr"):
            vals, flags = SM.long_vals(wp, k, W, D), SM.path_flags(W, 0)
            if W < 2:
                assert SM.solve_block(vals, flags, [], 0) is None and SM.solve_dense(vals, flags, [], 0) is None
                continue
            dts = SM.long_durations(D, mode, k)
            assert np.array_equal(bits(SM.solve_block(vals, flags, dts, 0)), bits(SM.solve_dense(vals, flags, dts, 0))), (k, W, mode)
            seen.add((W, SM.long_pattern(k)))
    assert {w for w, _ in seen} == {2, 3, 8, 9, 16, 17, 24, 32, 33} and len(seen) == 27


def flag_cases():
    """The inputs of tests/test_gpu_solve.py::test_waypoint_flags (K = 5, W = 5, so = 2, D = 3), built as there."""
    D, W, Kf = 3, 5, 5
    P, V, A = SM.USE_POS, SM.USE_VEL, SM.USE_ACC
    flags = np.array([[7, P, P, P, 7], [7, P | V, P | V, P | V, 7], [7, P, V, P, 7], [7, P, P | V, P, P | V],
                      [V | A, V | A, V | A, V | A, V | A]], np.uint8).T.copy()
    rng = np.random.default_rng(9)
    wp = np.zeros((14, W, Kf))
    for k in range(Kf):
        wp[:D, :, k] = SM.random_path(rng, W, D).T
    wp[D:3 * D] = np.round(rng.uniform(-1, 1, (2 * D, W, Kf)), 2)
    dts = np.round(rng.uniform(0.4, 1.8, (W - 1, Kf)), 3)
    dts[:, 4] = [1.0, 2.0, 0.5, 1.0]
    return wp, flags, dts


@pytest.mark.parametrize("inputs", [flag_cases, SM.long_flag_problems], ids=["W5", "W17"])
def test_block_twin_with_waypoint_flags(inputs):
    wp, flags, dts = inputs()
    W, D = wp.shape[1], 3
    for k in range(4):
        ratio = block_ratio(SM.long_vals(wp, k, W, D), flags[:, k], dts[:, k], 2, "flags problem %d" % k)
        print("solve_block, flags problem %d (W = %d): ratio %.3f" % (k, W, ratio))
    # no fixed position anywhere: singular in exact arithmetic, and an exact zero pivot in the twin
    vals = SM.long_vals(wp, 4, W, D)
    assert SM.solve_exact(vals, flags[:, 4], dts[:, 4], 2) is None and SM.solve_block(vals, flags[:, 4], dts[:, 4], 2) is None


def test_block_twin_reports_what_the_kernel_reports():
    name, vals, dts = CASES[2]
    flags = SM.path_flags(vals.shape[1], 2)
    assert SM.solve_block(vals[:, :1], flags[:1], [], 2) is None  # EMPTY
    for bad in (0.0, -0.4, np.nan, np.inf):  # BAD_TIME
        d = np.array(dts, dtype=np.float64)
        d[-1] = bad
        assert SM.solve_block(vals, flags, d, 2) is None
