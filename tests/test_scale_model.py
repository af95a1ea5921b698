"""tests/scale_model.py against the reference's recorded results (tests/golden/scale_golden.npz), against exact arithmetic,
and against a host build of csrc/mplx_scale_math.h (no GPU).

Golden.  Fed the golden's own LambdaSeg::a, the model's dT, Ts and total equal the golden bit for bit (lambda.h:57-60,
127-138 are IEEE arithmetic).  Its REFERENCE getTau finds a root exactly where the reference's did -- the lost end points
included: 0, total and 9 * (total / 9) -- and where both found one, tau and every sample row obey

    e_model <= 8 * max(e_ref, 2^-52 * scale)

with e = |value - truth|, truth from the exact root of the segment's quartic (scale_model.exact_tau), e_ref the
reference's own error and scale = tf for tau, |truth| for a row: the convention of tests/test_gpu_limits.py for results of
a different but equivalent evaluation (here: another libm's cbrt / acos / cos).  A sample whose root the reference lost
is the START state evaluated with lambda(0): IEEE arithmetic, bit for bit.  Where tau == tf, Lambda::evaluate finds no
segment and the reference reads a VirtualPoint it never initialised: the vel / acc / jrk rows of that Command are not
compared (the device defines lambda = lambda_dot = 0 there).  The model's own coefficients (the Hermite tree
of include/mplx_scale.h, not Eigen's inverse) are held to 8 * max(the golden's error, 2^-52 |a|) against the exact
Hermite cubic, and every coefficient sits a factor 2 away from the reference's 1e-5 clamp, so no clamp decision can
differ.

ROBUST, on 2 000 seeded scale(ri, rf) calls with 25 times each, the ends included: |getT(tau) - t| <= 8 * 2^-52 * total
(2.10 at worst with LAMBDA_NEWTON = 3 steps; the test prints the figure), tau is
non-decreasing in t, tau(0) == 0 and tau(total) == taus[S] exactly.

The shared header.  tests/sanitize/scale_math_harness.cpp, a stand-alone program, compiles csrc/mplx_scale_math.h with
g++ -fsanitize=address,undefined, runs the sweep in both modes and must agree with the model bit for bit on every value
that passes through no cbrt / acos / cos: the segment, the total, lambda and lambda_dot at its own tau, every tau of a
call with ri == rf (the linear branch of solve); its other taus obey the residual bound (ROBUST) or equal the model's
found flag (REFERENCE)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import limits_model as LM
import scale_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
FACTOR = 8.0
F = np.float64
REF, ROB = SM.REFERENCE, SM.ROBUST
CASES = [(D, S) for D in (2, 3) for S in (1, 3, 5)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(x, want):
    return np.array_equal(bits(x), bits(want))


@functools.lru_cache(maxsize=None)
def golden(D, S):
    g = np.load(os.path.join(ROOT, "tests", "golden", "scale_golden.npz"))
    name = "d%d_s%d/" % (D, S)
    return {k[len(name):]: g[k].view(np.float64) for k in g.files if k.startswith(name)}


def taus_of(dts):
    t = [F(0.0)]
    for d in dts:
        t.append(F(d) + t[-1])  # trajectory.h:54
    return np.array(t)


def query_times(total):
    """The driver's: total (i + 1/2) / 8, then 0, total, 9 * (total / 9)."""
    total = F(total)
    return [total * (i + 0.5) / 8 for i in range(8)] + [F(0.0), total, F(9) * (total / F(9))]


@pytest.mark.parametrize("D,S", CASES, ids=lambda x: str(x))
def test_model_against_golden(D, S):
    g = golden(D, S)
    K = g["a"].shape[0]
    worst_tau, worst_row, lost, clamped = 0.0, 0.0, 0, 0
    for k in range(K):
        taus = taus_of(g["dts"][k])
        T = taus[-1]
        a, ri, rf = g["a"][k], g["ri"][k], g["rf"][k]
        seg = SM.seg_from_a(a, F(0.0), T)
        assert same(seg[7], g["dT"][k, 0]), (k, "dT")
        lam = SM.Lambda([seg], REF)
        Ts = np.array([lam.getT(x) for x in taus])
        assert same(Ts, g["Ts"][k]), (k, "Ts")
        total = Ts[-1]
        assert same(total, g["total"][k, 0]), (k, "total")

        # the model's own coefficients against the exact Hermite cubic, and the clamp decisions
        pts = SM.scale_points(ri, rf, T)
        exact = SM.exact_hermite(pts[0][0], 0.0, 0.0, pts[0][1], 0.0, T)
        mine = SM.scale(taus, ri, rf, REF)
        assert mine["status"] == 0
        for i in range(4):
            x = abs(float(exact[i]))
            assert x < 0.5e-5 or x > 2e-5, "coefficient %d of trajectory %d sits within a factor 2 of the clamp: %g" % (i, k, x)
            want = 0.0 if x < 1e-5 else exact[i]
            clamped += x != 0 and x < 1e-5
            e_gold, e_mine = SM.err(a[i], want), SM.err(mine["lam"].segs[0][i], want)
            assert e_mine <= FACTOR * max(e_gold, EPS * x), (k, i, e_mine, e_gold)

        # getTau: found flags, and tau against the exact root
        for q, t in enumerate(query_times(total)):
            tau, found = lam.get_tau_reference(t)
            assert found == bool(g["found"][k, q]), "trajectory %d, time %d: found %r, the reference %r" % (k, q, found, g["found"][k, q])
            if not found:
                assert tau == -1 and g["tau"][k, q] == -1
                lost += 1
                continue
            truth = SM.exact_tau(seg, 0.0, t, near=g["tau"][k, q])
            assert truth is not None
            e_ref, e_mod = SM.err(g["tau"][k, q], truth), SM.err(tau, truth)
            worst_tau = max(worst_tau, e_mod / max(e_ref, EPS * float(T)))
            assert e_mod <= FACTOR * max(e_ref, EPS * float(T)), (k, q, e_mod, e_ref)

        # sample(9): Commands and Waypoints
        coef = g["coeff"][k][:, :D, :]
        cyaw = g["coeff"][k][:, D, :]
        step = total / F(9)
        for i in range(10):
            t = F(i) * step
            tau, raw, found, l, ld = lam.sample_tau(t, total, T)
            cmd = SM.sample_rows(coef, cyaw, taus, tau, l, ld, t, True)
            way = SM.sample_rows(coef, cyaw, taus, tau, l, ld, t, False)
            if not found:  # the START state with lambda(0)
                assert same(cmd, g["cmd"][k, i]) and same(way, g["way"][k, i]), (k, i)
                continue
            truth = SM.exact_tau(seg, 0.0, t, near=raw)
            tt, tl, tld = lam.clamp_eval(F(float(truth)), total, T)
            for rows, gold, command in ((cmd, g["cmd"][k, i], True), (way, g["way"][k, i], False)):
                true_rows = SM.sample_rows(coef, cyaw, taus, tt, tl, tld, t, command)
                fin = np.ones(rows.shape, bool)
                if command and not (tau >= seg[4] and tau < seg[5] and tt < seg[5]):
                    # Lambda::evaluate found no segment (tau == tf, here or at the exact root): the reference divides by a VirtualPoint it never
                    # initialised, so its vel / acc / jrk are whatever the stack held; the rows without lambda still count
                    fin[D:4 * D] = False
                e_ref, e_mod = np.abs(gold[fin] - true_rows[fin]), np.abs(rows[fin] - true_rows[fin])
                bound = FACTOR * np.maximum(e_ref, EPS * np.maximum(np.abs(true_rows[fin]), 1e-300))
                ratio = float(np.max(e_mod / np.maximum(bound / FACTOR, 1e-300)))
                worst_row = max(worst_row, ratio)
                assert (e_mod <= bound).all(), (k, i, command, rows, gold, true_rows)
    print("D %d S %d: worst tau ratio %.3f, worst row ratio %.3f, %d lost end points, %d clamped coefficients" % (D, S, worst_tau, worst_row, lost, clamped))
    assert lost > 0  # the reference's end points are lost in this fixture too
    if S == 5:
        assert clamped > 0  # the long trajectory


def test_golden_has_the_cases_the_fixture_promises():
    for D, S in CASES:
        g = golden(D, S)
        assert g["a"].shape[0] == 12
        assert (g["ri"] == g["rf"]).sum() >= 1
        assert ((g["ri"] >= 0.25) & (g["ri"] <= 4) & (g["rf"] >= 0.25) & (g["rf"] <= 4)).all()
        if S == 5:
            assert max(float(taus_of(d)[-1]) for d in g["dts"]) > 60


@functools.lru_cache(maxsize=None)
def robust_sweep():
    """Per call of the sweep: (result of scale in ROBUST mode, the 25 times, the 25 taus).  Computed once, shared."""
    T, ri, rf = SM.sweep()
    out = []
    for n in range(SM.N_SWEEP):
        taus = np.array([F(0.0), F(T[n])])
        r = SM.scale(taus, ri[n], rf[n], ROB)
        ts = SM.sweep_times(r["total"])
        out.append((r, ts, [r["lam"].get_tau_robust(t, r["total"], taus[-1]) for t in ts]))
    return out


def test_robust_inverse_on_the_sweep():
    T, ri, rf = SM.sweep()
    worst = 0.0
    for n, (r, ts, tau) in enumerate(robust_sweep()):
        assert r["status"] == 0
        lam, total = r["lam"], r["total"]
        assert tau[0] == 0.0 and same(tau[-1], T[n]), n
        for q, (t, x) in enumerate(zip(ts, tau)):
            res = abs(float(lam.getT(x)) - float(t)) / (EPS * float(total))
            worst = max(worst, res)
            assert res <= FACTOR, "call %d (T %g, ri %g, rf %g), time %d: |getT(tau) - t| = %.2f * 2^-52 * total" % (n, T[n], ri[n], rf[n], q, res)
            assert q == 0 or x >= tau[q - 1], (n, q)
    print("worst |getT(tau) - t| / (2^-52 total) after %d Newton steps: %.3f" % (SM.NEWTON, worst))


def test_statuses_of_the_model():
    good = ([1.0, 2.0, 1.5], [0.0, 0.1, 0.0], [0.0, 1.0, 3.0])
    assert SM.build_lambda(*good, ROB)[1] == 0 and SM.build_lambda(*good, REF)[1] == 0
    for mode in (REF, ROB):
        assert SM.build_lambda([1.0], [0.0], [0.0], mode)[1] == SM.BAD_POINTS
        assert SM.build_lambda([1.0] * 10, [0.0] * 10, list(range(10)), mode)[1] == SM.BAD_POINTS
        assert SM.build_lambda([1.0, np.nan], [0.0, 0.0], [0.0, 1.0], mode)[1] == SM.BAD_POINTS
        assert SM.scale(np.array([0.0, 2.0]), -1.0, 1.0, mode)["status"] == SM.BAD_POINTS
        assert SM.scale(np.array([0.0, 2.0]), 1.0, np.inf, mode)["status"] == SM.BAD_POINTS
        assert SM.scale(np.array([0.0, 2.0]), np.nan, 1.0, mode)["status"] == SM.BAD_POINTS
    assert SM.build_lambda([1.0, 2.0], [0.0, 0.0], [1.0, 1.0], ROB)[1] == SM.BAD_POINTS      # times do not grow
    assert SM.build_lambda([1.0, 0.0], [0.0, 0.0], [0.0, 1.0], ROB)[1] == SM.BAD_POINTS      # p <= 0
    assert SM.build_lambda([1.0, 0.0], [0.0, 0.0], [0.0, 1.0], REF)[1] == 0                  # ... which the reference takes
    # positive at both ends, negative in between: the slope dives
    assert SM.build_lambda([0.5, 0.5], [-4.0, 4.0], [0.0, 1.0], ROB)[1] == SM.NOT_POSITIVE
    assert SM.build_lambda([0.5, 0.5], [-4.0, 4.0], [0.0, 1.0], REF)[1] == 0
    # a3 == 0: the quadratic's single extremum, through the linear root
    lam, st = SM.build_lambda([1.0, 1.0], [-3.0, 3.0], [0.0, 2.0], ROB)
    assert st == SM.NOT_POSITIVE  # lambda = 1 - 3 t + 1.5 t^2: -0.5 at t = 1
    # the clamp of REFERENCE breaks a long trajectory: lambda(T) is wrong by far more than 0.1 %
    r = SM.scale(np.array([0.0, 64.0]), 1.0, 2.0, REF)
    l_end = SM.seg_lambda(r["lam"].segs[0][:4], F(64.0))
    assert abs(float(l_end) - 0.5) > 0.5e-3
    r = SM.scale(np.array([0.0, 64.0]), 1.0, 2.0, ROB)
    assert abs(float(SM.seg_lambda(r["lam"].segs[0][:4], F(64.0))) - 0.5) < 1e-12


# ------------------------------------------------------------------------------------------------------ scale_down
def crafted(D, T=2.0, peak=3.0):
    """One segment per axis pattern: axis 0 the crafted quintic, the others at rest."""
    return [[SM.crafted_quintic(peak, T)] + [np.zeros(6)] * (D - 1)], [T]


def test_scale_down_on_crafted_quintics():
    T, peak, mv = 2.0, 3.0, 1.5
    coefs, dts = crafted(2, T, peak)
    taus = taus_of(dts)
    r = SM.scale_down(coefs, dts, taus, mv, 0.0, 0.0, 0.0, ROB)
    # velocity only: the single peak at T / 2, l = peak / mv exactly (dyadic inputs, the root of a cubic through cbrt /
    # acos / cos: the tolerance of the limits model, 2 * 2^-52 * scale with scale = the sum of |terms| of v at T / 2)
    scale = LM.scale_of(coefs[0][0], T / 2, 1)
    assert r["scaled"] == 1 and r["status"] == 0
    assert abs(float(r["max_l"]) - peak / mv) <= 2 * EPS * scale / mv
    assert abs(float(r["t_lo"]) - T / 2) < 1e-9 and same(r["t_lo"], r["t_hi"])
    # ri = rf = 0: a uniform scaling -- every point has p = max_l, and every sample is within the limit, reaching it at the peak
    p, t = r["points"]
    assert all(same(x, r["max_l"]) for x in p) and len(p) == 3 and t[0] == 0 and same(t[-1], T)
    lam, total = r["lam"], r["total"]
    top = 0.0
    for i in range(65):
        tt = F(i) * (total / F(64))
        tau, raw, found, l, ld = lam.sample_tau(tt, total, taus[-1])
        row = SM.sample_rows([coefs[0]], [np.zeros(6)], taus, tau, l, ld, tt, True)
        v = np.abs(row[2:4]).max()
        assert v <= mv * (1 + 4 * EPS), (i, v)
        top = max(top, float(v))
    assert abs(top - mv) <= 2 * EPS * scale  # sample 32 is the peak

    # acceleration: |a| peaks at T (1/2 -+ 1/(2 sqrt 3)) with 16 peak / (3 sqrt(3) T); l = sqrt(|a| / ma)
    a_peak = 16 * peak / (3 * np.sqrt(3.0) * T)
    ma = a_peak / 4
    r = SM.scale_down(coefs, dts, taus, 0.0, ma, 0.0, 0.0, ROB)
    assert r["scaled"] == 1 and abs(float(r["max_l"]) - 2.0) < 1e-12
    assert abs(float(r["t_lo"]) - T * (0.5 - 0.5 / np.sqrt(3.0))) < 1e-12 and abs(float(r["t_hi"]) - T * (0.5 + 0.5 / np.sqrt(3.0))) < 1e-12
    lam, total = r["lam"], r["total"]
    for i in range(65):
        tt = F(i) * (total / F(64))
        tau, raw, found, l, ld = lam.sample_tau(tt, total, taus[-1])
        row = SM.sample_rows([coefs[0]], [np.zeros(6)], taus, tau, l, ld, tt, True)
        assert np.abs(row[4:6]).max() <= ma * (1 + 4 * EPS), i

    # both limits: the larger l wins; ramps at both ends with lambda 1 there
    r = SM.scale_down(coefs, dts, taus, mv, ma, 1.0, 1.0, ROB)
    assert r["scaled"] == 1 and same(r["max_l"], max(F(peak) / F(mv), r["max_l"])) and r["lam"].n == 3
    p, t = r["points"]
    assert p[0] == 1.0 and p[-1] == 1.0 and len(p) == 4

    # within the limits: left unscaled
    assert SM.scale_down(coefs, dts, taus, 2 * peak, 2 * a_peak, 0.0, 0.0, ROB)["scaled"] == 0
    assert SM.scale_down(coefs, dts, taus, 0.0, 0.0, 0.0, 0.0, ROB)["scaled"] == 0  # nothing is checked


def test_scale_down_over_segments():
    """Two segments; the second one breaks the limit at its start and at its end: 0 is a candidate for s != 0, a violation
    at T wins over rf."""
    c0 = np.array([0, 0, 0, 0, 1.0, 0.0])           # v = 1
    c1 = np.array([0, 0, 0, 0, 3.0, 1.0])           # v = 3 throughout
    coefs, dts = [[c0, np.zeros(6)], [c1, np.zeros(6)]], [1.0, 2.0]
    taus = taus_of(dts)
    r = SM.scale_down(coefs, dts, taus, 2.0, 0.0, 1.0, 1.0, ROB)
    assert r["scaled"] == 1 and r["max_l"] == 1.5 and r["t_lo"] == 1.0 and r["t_hi"] == 3.0
    p, t = r["points"]
    assert [float(x) for x in p] == [1.0, 1.5, 1.5] and [float(x) for x in t] == [0.0, 1.0, 3.0]


# ---------------------------------------------------------------------------------------- the shared math header
def test_math_header_under_asan_ubsan_agrees_with_the_model(tmp_path):
    # (no skip without g++: this is the only sanitizer run of the header and the only CPU check that it equals the model;
    # the golden generator needs the same compiler)
    exe = str(tmp_path / "scale_math_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-ffp-contract=off",
           "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "sanitize", "scale_math_harness.cpp")]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    T, ri, rf = SM.sweep()
    Q = SM.SWEEP_TIMES
    n = SM.N_SWEEP
    # ROBUST: scale_model.sweep_times; REFERENCE: total (i + 1/2) / 25
    rows = []
    for mode in (ROB, REF):
        fr = [-(i + 1.0) for i in range(Q - 1)] + [1.0] if mode == ROB else [(i + 0.5) / Q for i in range(Q)]
        for k in range(n):
            rows.append([T[k], ri[k], rf[k], float(mode)] + fr)
    ipath, opath = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([[2.0 * n, float(Q)], np.asarray(rows).ravel()]).tofile(ipath)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, ipath, opath], capture_output=True, text=True, timeout=600, env=env)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "harness: ok" in run.stdout
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
    out = np.fromfile(opath, dtype=np.float64).reshape(2 * n, 10 + 6 * Q)
    sweep_rob = robust_sweep()
    worst, left_out = 0.0, 0
    for mode, base in ((ROB, 0), (REF, n)):
        for k in range(n):
            o = out[base + k]
            taus = np.array([F(0.0), F(T[k])])
            r = sweep_rob[k][0] if mode == ROB else SM.scale(taus, ri[k], rf[k], REF)
            lam, total = r["lam"], r["total"]
            assert o[0] == 0 and same(o[1:9], lam.segs[0]) and same(o[9], total), (mode, k)
            per = o[10:].reshape(Q, 6)
            ieee_only = ri[k] == rf[k]
            for q in range(Q):
                t, raw, found, tau, l, ld = per[q]
                want_t = sweep_rob[k][1][q] if mode == ROB else total * F((q + 0.5) / Q)
                assert same(t, want_t), (mode, k, q)
                # lambda and lambda_dot at the program's own tau: IEEE arithmetic
                tt, tl, tld = lam.clamp_eval(F(raw), total, taus[-1])
                assert same(tau, tt) and same(l, tl) and same(ld, tld), (mode, k, q)
                if mode == ROB:
                    m_raw = sweep_rob[k][2][q]
                    assert found == 1
                    if ieee_only or q == 0 or q == Q - 1:
                        assert same(raw, m_raw), (k, q)
                    res = abs(float(lam.getT(F(raw))) - float(t)) / (EPS * float(total))
                    worst = max(worst, res)
                    assert res <= FACTOR, (k, q, res)
                else:
                    m_raw, m_found, seg_id, libm = lam.get_tau_reference(t, want_info=True)
                    if not libm:
                        assert same(raw, m_raw) and bool(found) == m_found, (k, q)
                        continue
                    near = m_found and min(abs(float(m_raw)), abs(float(m_raw) - T[k])) <= 1e-9
                    if near:
                        left_out += 1
                        continue
                    assert bool(found) == m_found, (k, q)
                    if m_found:
                        truth = SM.exact_tau(lam.segs[0], 0.0, t) if (k % 50 == 0) else None  # the 8 x rule on a sample of the calls
                        if truth is not None:
                            assert SM.err(raw, truth) <= FACTOR * max(SM.err(m_raw, truth), EPS * T[k]), (k, q)
    print("harness: worst robust residual %.3f * 2^-52 * total; %d reference cases left out (root within 1e-9 of an end)" % (worst, left_out))
    assert left_out <= 0.02 * n * Q
