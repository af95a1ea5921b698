"""CPU: tests/heur_model.py, the restatement of include/mplx_heur.h -- its REFERENCE mode against the reference's own
cal_heur (tests/golden/heur_golden.npz, bit for bit), its ROBUST mode against the exact minimum in extended precision,
the shared header csrc/mplx_heur_math.h against both (a stand-alone program under ASan + UBSan), and the host planner
with the setter on against the reference's MapPlanner (the golden known-answer plan), through the CPU oracle's lists.

The tolerance of ROBUST.  profiles/micro/heur_dyn_error.py measured the worst |h - h*| on 50 000 states per branch in
units of u = 2^-52 * sum |terms of C at the minimiser| (profiles/heur_dyn_error.json, DESIGN.md 4.23: worst_units);
the tests assert 8 x that figure, the margin DESIGN.md 4.17 uses for the same kind of quantity."""
import json
import os
import subprocess

import numpy as np
import pytest

import heur_model as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "heur_golden.npz")
MEASURED = json.load(open(os.path.join(ROOT, "profiles", "heur_dyn_error.json")))
TOL_UNITS = 8.0 * MEASURED["worst_units"]
F = np.float64


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def golden_cases():
    z = np.load(GOLD)
    names = sorted({k.split("/")[0] for k in z.files if k.startswith("d")})
    for name in names:
        D, cs, cg = int(name[1]), int(name[3:5], 16), int(name[6:8], 16)
        w, v_max = z[name + "/setting"].view(np.float64)
        yield name, D, cs, cg, float(w), float(v_max), z[name + "/goal"].view(np.float64), z[name + "/states"].view(np.float64), \
            z[name + "/h"].view(np.float64), z[name + "/n_roots"]


def test_reference_mode_equals_the_reference_bit_for_bit():
    n = no_root = dbl_max = zero_dp = 0
    for name, D, cs, cg, w, v_max, goal, s, h, n_roots in golden_cases():
        got = np.array([HM.reference(s[:, k], goal, cs, cg, w, v_max, D) for k in range(s.shape[1])])
        assert np.array_equal(bits(got), bits(h)), name
        n += s.shape[1]
        no_root += int((n_roots == 0).sum())
        dbl_max += int((h > 1e300).sum())
        zero_dp += int(np.all(s[:D] == goal[:D, None], axis=0).sum())
    print("golden: %d states, quartic without a root %d, DBL_MAX returned %d, dp = 0 %d" % (n, no_root, dbl_max, zero_dp))
    assert n >= 2 * 5 * 2 * 200 and no_root >= 3 and dbl_max >= 3 and zero_dp >= 100
    assert HM.reference(np.zeros(9), np.zeros(9), HM.JRK, HM.JRK, 1.0, 1.0, 2) is None  # the Eigen-solver branches


@pytest.fixture(scope="module")
def sweeps():
    """Per branch 160 columns in 2-D and 3-D under two settings, a quarter of them pre-selected for three stationary
    points; the exact minima once, shared by the tests below."""
    out = []
    for bi, branch in enumerate(HM.BRANCHES):
        for D, (w, v_max) in ((2, HM.SWEEP_SETTINGS[0]), (3, HM.SWEEP_SETTINGS[2])):
            s, goal = HM.sweep_states(branch, D, 80, 31 * bi + D, three_share=0.25)
            out.append((branch, D, w, v_max, s, goal, HM.sweep_units(branch, D, s, goal, w, v_max)))
    return out


def test_robust_mode_is_the_exact_minimum(sweeps):
    worst, three, bar, interior, zero_dp = 0.0, 0, 0, 0, 0
    for branch, D, w, v_max, s, goal, rows in sweeps:
        for k, (u, npos, where, h, hs, scale) in enumerate(rows):
            assert u <= TOL_UNITS, (branch, D, k, u, h, hs)
            worst = max(worst, u)
            three += npos >= 3
            bar += where == "bar"
            interior += where == "interior"
        zero_dp += int(np.all(s[:D] == goal[:D, None], axis=0).sum())
    print("worst %.3f units (tolerance %.3f), three stationary points %d, minimum at t_bar %d, interior %d, dp = 0 %d"
          % (worst, TOL_UNITS, three, bar, interior, zero_dp))
    assert three >= 50 and bar >= 50 and interior >= 50 and zero_dp >= 10


def test_robust_mode_bounds(sweeps):
    """Never below the default, bit for bit; never above C(t) at any t >= t_bar; and how often REFERENCE is above it."""
    rng = np.random.default_rng(3)
    ref_above = ref_total = 0
    for branch, D, w, v_max, s, goal, rows in sweeps:
        cs, cg = branch
        h = HM.robust(s, goal, cs, cg, w, v_max, D)
        d = HM.default_heur(s, [F(x) for x in goal], F(w), F(v_max), D)
        assert np.all(h >= d)
        assert np.array_equal(bits(h[h <= d]), bits(d[h <= d]))  # where the dynamics add nothing: the default's bits
        g = [F(x) for x in goal]
        co = HM.coefficients(s, g, cs, cg, F(w), D)
        cost = (lambda t: co[1] / t + w * t) if co[0] == "vel" else HM.cost_acc(co[1], co[2], co[3], F(w)) if co[0] == "acc" \
            else HM.cost_jrk(F(w), *co[1:])
        t_bar = HM._linf(s, g, D) / F(v_max)
        at_min = np.array([r[5] for r in rows])  # sum |terms| at the minimiser: the unit of h's own error
        terms = HM.abs_terms(co, F(w))
        for _ in range(64):  # t_bar itself, then times above it up to five-fold
            t = np.maximum(t_bar, 1e-3) * (1.0 + (4.0 * rng.random(s.shape[1]) ** 2 if _ else 0.0))
            with np.errstate(all="ignore"):
                c, unit = np.maximum(cost(t), d), terms(t) + at_min
            assert np.all(h <= c + TOL_UNITS * 2.0 ** -52 * unit), (branch, D)
        if cs == HM.ACC:
            for k in range(s.shape[1]):
                r = HM.reference(s[:, k], goal, cs, cg, w, v_max, D)
                ref_total += 1
                ref_above += r > h[k] * (1 + 1e-9) + 1e-12
    print("REFERENCE above ROBUST on %d of %d ACC states (reported, not asserted)" % (ref_above, ref_total))


def test_special_values():
    g = np.zeros(10)
    s = np.zeros((10, 4))
    s[2, 1] = 1.0          # dp = 0 with a live velocity: the cost of stopping and coming back
    s[0, 2] = np.nan
    s[0, 3] = 2.0
    h = HM.robust(s, g, HM.ACC, 0, 1.0, 2.0, 2)
    assert h[0] == 0.0 and h[1] > 0.0 and np.isnan(h[2]) and h[3] > 1.0
    assert np.isnan(HM.robust(s, g, HM.ACC, 0, np.inf, 2.0, 2)).all()
    hv = HM.robust(s, g, HM.ACC, 0, 1.0, 0.0, 2)  # v_max <= 0: t_bar = 0, the default is w * Linf
    assert hv[3] >= 2.0 and hv[0] == 0.0
    assert np.array_equal(bits(HM.robust(s, g, HM.SNP, 0, 1.0, 2.0, 2)[[0, 1, 3]]), bits(HM.default_heur(s, g, F(1.0), F(2.0), 2)[[0, 1, 3]]))
    # rest to rest, ACC-ACC, far from t_bar: the textbook value min_t 12 dp^2 / t^3 + w t = (4/3) (36 dp^2 w^3)^(1/4)
    assert abs(h[3] - 4.0 / 3.0 * (36.0 * 4.0) ** 0.25) < 1e-12


# ---------------------------------------------------------------------------------------- the shared math header
def test_math_header_under_asan_ubsan_agrees_with_the_model(tmp_path):
    exe = str(tmp_path / "heur_math_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "sanitize", "heur_math_harness.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    ipath, opath = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")

    def harness(D, cs, cg, mode, w, v_max, goal, s):
        n = 4 * D + 1
        np.concatenate([[D, cs, cg, mode, w, v_max, s.shape[1]], goal[:n], s[:n].T.ravel()]).astype(np.float64).tofile(ipath)
        run = subprocess.run([exe, ipath, opath], capture_output=True, text=True, timeout=600, env=env)
        assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
        assert "harness: ok" in run.stdout and "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
        return np.fromfile(opath, dtype=np.float64)

    for name, D, cs, cg, w, v_max, goal, s, h, n_roots in golden_cases():  # REFERENCE: the header is the reference
        assert np.array_equal(bits(harness(D, cs, cg, HM.REFERENCE, w, v_max, goal, s)), bits(h)), name
    rng = np.random.default_rng(9)
    pairs = HM.BRANCHES + [(HM.ACC | HM.YAW, HM.ACC), (HM.SNP, HM.SNP), (HM.VEL, HM.ACC), (HM.JRK, 0)]
    for D in (2, 3):
        for cs, cg in pairs:
            for w, v_max in ((1.0, 2.0), (10.0, 3.0), (0.5, 0.0), (2.0, -1.0)):
                s = HM.lattice_states(rng, 120, D, min(cs & 15, HM.JRK), zero_dp=0.1)
                s[D, 5], s[0, 6] = np.nan, np.inf
                goal = HM.sweep_goal(D, (cg or cs) & 15)
                want = HM.robust(s, goal, cs, cg, w, v_max, D)
                got = harness(D, cs, cg, HM.ROBUST, w, v_max, goal, s)
                nan = np.isnan(want)
                assert nan[5] and nan[6] and np.array_equal(np.isnan(got), nan), (D, cs, cg)
                assert np.array_equal(bits(got[~nan]), bits(want[~nan])), (D, cs, cg, w, v_max)


# ---------------------------------------------------------------------------------------- the host planner
def corridor_planner(engine, ignore, robust=False, lpa=False):
    from oracle import oracle as O
    from test_plan_known_answer import corridor, provider_from_oracle
    m = engine
    c = corridor()
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)  # test_planner_2d.cpp:49-53
    oenv = O.Env(2, O.ACC, U, c["cells"], c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    prov, keep = provider_from_oracle(oenv)
    planner = m.MapPlanner(2, provider=prov)
    mu = m.MapUtil(2)
    mu.setMap(c["origin"], c["dim"], c["cells"], c["res"])
    planner.setMapUtil(mu)
    planner.setVmax(1.0)
    planner.setAmax(1.0)
    planner.setDt(1.0)
    planner.setU(U)
    if lpa:
        planner.setLPAstar(True)
    planner.setHeurIgnoreDynamics(ignore, robust)
    start = m.Waypoint(2, m.ACC, pos=c["start"])
    goal = m.Waypoint(2, m.ACC, pos=c["goal"])
    return planner, start, goal, keep


def test_planner_with_the_setter_on_reproduces_the_reference_plan(engine):
    """MapPlanner.setHeurIgnoreDynamics(False) on the corridor of test_planner_2d: cost, expanded states and duration of
    the reference's own MapPlanner with the setter on.  (Its cost, 352.0, is above the optimum 351.5: the heuristic is
    not admissible for a goal region.)"""
    z = np.load(GOLD)
    assert int(z["plan/ok"][0]) == 1
    planner, start, goal, keep = corridor_planner(engine, False)
    assert planner.plan(start, goal)
    s = planner.summary()
    print("REFERENCE:", s["cost"], s["expansions"], planner.getTraj().getTotalTime())
    assert s["cost"] == z["plan/cost"].view(np.float64)[0] and s["expansions"] == int(z["plan/expanded"][0])
    assert planner.getTraj().getTotalTime() == z["plan/duration"].view(np.float64)[0] and s["segments"] == int(z["plan/segments"][0])
    planner.setHeurIgnoreDynamics(True)
    assert planner.plan(start, goal) and planner.summary()["cost"] == 351.5
    default_expansions = planner.summary()["expansions"]
    planner.setHeurIgnoreDynamics(False, robust=True)
    assert planner.plan(start, goal)
    r = planner.summary()
    print("ROBUST:", r["cost"], r["expansions"], "default:", default_expansions)
    # (the corridor's goal is a box of 0.5 m with a free velocity: no fixed-goal bound is admissible there, and ROBUST
    # says so in include/mplx_heur.h section 3; the exact-goal scenario of tests/test_gpu_heur_plan.py is where it is)
    assert r["cost"] >= 351.5 and r["segments"] == 35
    planner.close()
    del keep


def test_planner_refusals(engine):
    m = engine
    A = m._abi
    planner, start, goal, keep = corridor_planner(engine, True)
    L = A.lib()
    assert L.mplx_planner_set_heur_dynamics(None, 0) == A.ERR_ARG
    assert L.mplx_planner_set_heur_dynamics(planner._p, 3) == A.ERR_ARG
    planner.setHeurIgnoreDynamics(False)  # REFERENCE on a JRK state space: refused by plan()
    js, jg = m.Waypoint(2, m.JRK, pos=start.pos), m.Waypoint(2, m.JRK, pos=goal.pos)
    with pytest.raises(A.MplxError) as e:
        planner.plan(js, jg)
    assert e.value.code == A.ERR_STATE
    planner.setW(0.0)
    with pytest.raises(A.MplxError) as e:
        planner.plan(start, goal)
    assert e.value.code == A.ERR_STATE
    planner.close()
    del keep
