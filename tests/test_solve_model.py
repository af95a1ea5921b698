"""CPU: the two models of the trajectory solver (tests/solve_model.py; include/mplx_solve.h) against each other and against
the statement of the problem, and the ctypes structs against the header.  No GPU.

solve_dense (poly_solver.cpp restated in float64) is held to solve_exact (the same statement in exact rationals) by a
bound that comes from the problem, not from either model: an LU solve of a system of order n loses at most about
n * eps * cond relative to its solution, and the dense solve chains two of them -- the free system Rpp and the
segment's own N x N block of A -- so |dense - exact| <= (n_free * cond_2(Rpp) + N * max_s cond_2(A_s)) * 2^-52 * scale,
with a floor of 64 * 2^-52 * scale (a handful of roundings per coefficient); scale is the largest exact coefficient."""
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
