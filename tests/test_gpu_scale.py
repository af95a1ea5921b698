"""Time scaling on the device (include/mplx_scale.h, csrc/scale_kernel.hip, the Lambda instantiations of
csrc/traj_kernel.hip) against tests/scale_model.py.

Bit for bit: everything a build writes (coefficients, ti, tf, getT(ti), dT, Ts, total, statuses: IEEE arithmetic), lambda
and lambda_dot at the device's own tau, and every sample row given the device's tau.  Held to a bound: tau itself, whose
closed-form start passes through the device library's cbrt / acos / cos.
  ROBUST:    |getT(tau) - t| <= 8 * 2^-52 * total with the model's getT, tau non-decreasing in t, tau(t <= 0) == 0 and
             tau(t >= total) == taus[S] exactly.
  REFERENCE: at t = total (i + 1/2) / 9, found as the model's and e_dev <= 8 * max(e_model, 2^-52 * tf) against the exact
             root next to the model's (scale_model.exact_tau); a case whose model root lies within 1e-9 of an end of
             its segment may be left out, at most 2 % of them.  The lost end points are pinned by
             tests/test_scale_model.py, not here.
  scale_down: max_l, t_lo, t_hi with the same rule against the exact extrema (limits_model.true_roots) where they pass
             through cbrt / acos / cos, bit for bit where the candidate is an end of a segment.
The worst ratios are printed (pytest -s).

Shapes: K = 70 (a wave and six lanes), w_max = 6 with S mixed 0 .. 5 (S = 0: a failed load, skipped everywhere), N = 9
uniform samples and a per-trajectory time column, D in {2, 3}; problem 11 lasts 64 s (the reference's clamp fires)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import limits_model as LM
import scale_model as SM
from test_gpu_solve import same_bits

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
FACTOR = 8.0
F = np.float64
K, WMAX, N = 70, 6, 9
LONG = 11
RATIOS = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0]
REF, ROB = SM.REFERENCE, SM.ROBUST
JRKxYAW = 0x17
FILL = 0xAB
FILL_F64 = np.frombuffer(bytes([FILL] * 8), dtype=np.float64)[0]
FILL_I32 = np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0]
MODES = [pytest.param(REF, id="reference"), pytest.param(ROB, id="robust")]


@functools.lru_cache(maxsize=None)
def times_of_set():
    """What does not depend on D, so the Lambdas (and their exact roots) are shared: n_segs [K], dts [5][K], ri, rf [K]."""
    rng = np.random.default_rng(77)
    n_segs = np.array([k % WMAX for k in range(K)], np.int32)
    dts = rng.integers(2, 13, (WMAX - 1, K)).astype(np.float64) / 4.0
    dts[:, LONG] = [16.0, 12.0, 16.0, 8.0, 12.0]
    ri, rf = rng.choice(RATIOS, K), rng.choice(RATIOS, K)
    same = ri == rf
    rf[same] = np.where(ri[same] == 4.0, 0.25, 4.0)
    rf[2] = ri[2]                    # the linear branch of solve
    ri[LONG], rf[LONG] = 1.0, 2.0    # 2 |dp| / T^3 = 3.8e-6: the clamp of REFERENCE
    ri[7], rf[13], ri[19], rf[25] = -1.0, np.nan, np.inf, 0.0   # MPLX_LAMBDA_BAD_POINTS in both modes
    return n_segs, dts, ri, rf


@functools.lru_cache(maxsize=None)
def coeff_of_set(D):
    """[5][D + 1][6][K] sixteenths in +-2; of the yaw primitive c(4), c(5) only; the long problem scaled down."""
    rng = np.random.default_rng(500 + D)
    c = rng.integers(-32, 33, (WMAX - 1, D + 1, 6, K)).astype(np.float64) / 16.0
    c[:, D, :4, :] = 0.0
    c[..., LONG] /= 64.0
    return c


def taus_of(dts, S):
    t = [F(0.0)]
    for s in range(S):
        t.append(t[-1] + F(dts[s]))
    return np.array(t)


def make_set(m, D, v_max=2.0, a_max=1.5):
    env = m.EnvMap(D)
    env.set_control(JRKxYAW)
    env.set_v_max(v_max)
    env.set_a_max(a_max)
    n_segs, dts, ri, rf = times_of_set()
    poly = env.load_traj(coeff_of_set(D), dts, n_segs=n_segs, control=JRKxYAW)
    assert (poly.status[n_segs == 0] == m.SOLVE_EMPTY).all() and (poly.status[n_segs > 0] == 0).all()
    return env, poly


@functools.lru_cache(maxsize=None)
def scale_models(mode):
    """Per problem None (S = 0) or what scale_model.scale returns; computed once, shared by every test and both D."""
    n_segs, dts, ri, rf = times_of_set()
    return [SM.scale(taus_of(dts[:, k], n_segs[k]), ri[k], rf[k], mode) if n_segs[k] else None for k in range(K)]


def check_build(d, models, n_segs, what, untouched):
    """The rows of a build against the model's, bit for bit.  untouched: what an entry the call does not own holds
    (the fill of the resident rows, or the zeros of the host form): status of a failed load, everything but the status
    of a problem with a Lambda status, rows past n_lseg / S_k."""
    u8, i32, f64 = untouched
    for k, r in enumerate(models):
        if r is None:
            assert d["status"][k] == u8 and d["n_lseg"][k] == i32, (what, k)
            same_bits(d["total"][k], f64, "%s: total of the failed load %d" % (what, k))
            same_bits(d["segs"][:, :, k], np.full((8, 8), f64), "%s: segs of the failed load %d" % (what, k))
            continue
        assert d["status"][k] == r["status"], (what, k, d["status"][k], r["status"])
        if r["status"]:
            assert d["n_lseg"][k] == i32, (what, k)
            same_bits(d["total"][k], f64, "%s: total of problem %d" % (what, k))
            same_bits(d["Ts"][:, k], np.full(WMAX, f64), "%s: Ts of problem %d" % (what, k))
            same_bits(d["segs"][:, :, k], np.full((8, 8), f64), "%s: segs of problem %d" % (what, k))
            continue
        lam, S = r["lam"], int(n_segs[k])
        assert d["n_lseg"][k] == lam.n, (what, k)
        same_bits(d["segs"][:lam.n, :, k], lam.segs, "%s: segments of problem %d" % (what, k))
        same_bits(d["segs"][lam.n:, :, k], np.full((8 - lam.n, 8), f64), "%s: rows past n_lseg of problem %d" % (what, k))
        same_bits(d["Ts"][:S + 1, k], r["Ts"], "%s: Ts of problem %d" % (what, k))
        same_bits(d["Ts"][S + 1:, k], np.full(WMAX - S - 1, f64), "%s: Ts past S of problem %d" % (what, k))
        same_bits(d["total"][k], r["total"], "%s: total of problem %d" % (what, k))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [2, 3])
def test_scale(engine, D, mode):
    m = engine
    env, poly = make_set(m, D)
    n_segs, dts, ri, rf = times_of_set()
    models = scale_models(mode)
    assert sum(r is not None and r["status"] == m.LAMBDA_BAD_POINTS for r in models) >= 3
    # the _device form on rows filled with a pattern: what it does not own keeps the caller's bytes
    rows = env.alloc_lambda_rows(K, WMAX)
    rows.fill(FILL)
    d_ri, d_rf = m.DeviceArray(env, K * 8), m.DeviceArray(env, K * 8)
    d_ri.upload(ri)
    d_rf.upload(rf)
    poly.scale_resident(rows, d_ri, d_rf, robust=mode == ROB)
    env.synchronize()
    check_build(rows.download(), models, n_segs, "scale_device", (FILL, FILL_I32, FILL_F64))
    # the host form: the same values, zeros where the call owns nothing
    h = poly.scale(ri, rf, robust=mode == ROB)
    check_build(h, models, n_segs, "scale", (0, 0, 0.0))
    seg = poly.lambda_segments()
    assert np.array_equal(seg["n_lseg"], h["n_lseg"]) and seg["a"].shape == (8, 4, K)
    # info reports the scaled total, the efforts stay
    info = poly.info()
    st = poly.segment_times()
    for k, r in enumerate(models):
        if r is None or r["status"]:
            same_bits(info["total_time"][k], poly.total_time[k], "unscaled total of problem %d" % k)
            assert not st[:, k].any()
            continue
        same_bits(info["total_time"][k], r["total"], "scaled total of problem %d" % k)
        same_bits(st[:n_segs[k], k], r["Ts"][1:] - r["Ts"][:-1], "segment times of problem %d" % k)
    poly.clear_lambda()
    same_bits(poly.info()["effort"], info["effort"], "efforts")
    # scalar ratios: every problem the same call
    h = poly.scale(2.0, 0.5, robust=mode == ROB)
    for k in (1, 5, LONG, K - 1):
        r = SM.scale(taus_of(dts[:, k], n_segs[k]), 2.0, 0.5, mode)
        same_bits(h["segs"][:1, :, k], r["lam"].segs, "scalar scale of problem %d" % k)
        same_bits(h["total"][k], r["total"], "scalar total of problem %d" % k)
    for b in (rows, d_ri, d_rf, poly):
        b.free()
    env.close()


@functools.lru_cache(maxsize=None)
def point_sets():
    """Caller-given Lambdas: p, v, t [9][K], n_pts [K].  Most problems: 9 points (8 segments) with non-zero v spanning
    [0, T]; then one of every status."""
    rng = np.random.default_rng(31)
    n_segs, dts, _, _ = times_of_set()
    p = np.round(rng.uniform(0.6, 2.0, (9, K)), 3)
    v = np.round(rng.uniform(-0.05, 0.05, (9, K)), 3)
    t = np.zeros((9, K))
    n_pts = np.full(K, 9, np.int32)
    for k in range(K):
        T = float(taus_of(dts[:, k], n_segs[k])[-1]) if n_segs[k] else 1.0
        n_pts[k] = 2 + (k % 8)
        cuts = np.sort(rng.uniform(0.1, 0.9, n_pts[k] - 2))
        t[:n_pts[k], k] = np.concatenate([[0.0], np.round(cuts * T, 3), [T]])
    n_pts[3] = 1                                 # too few
    n_pts[4] = 10                                # too many
    p[1, 8] = np.inf                             # not finite
    t[2, 9] = t[1, 9] - 0.125                    # times do not grow (n_pts[9] = 3)
    p[0, 10] = 0.0                               # p <= 0
    n_pts[14], p[:2, 14], v[:2, 14], t[:2, 14] = 2, [0.5, 0.5], [-4.0, 4.0], [0.0, 1.0]   # 0.5 - 4 s + 4 s^2: NOT_POSITIVE
    n_pts[16], p[:2, 16], v[:2, 16], t[:2, 16] = 2, [0.25, 1.0], [-3.0, 0.0], [0.0, 1.0]  # a cubic that dives: NOT_POSITIVE
    v[0, 15] = np.nan
    return p, v, t, n_pts


@pytest.mark.parametrize("mode", MODES)
def test_set_lambda(engine, mode):
    m = engine
    D = 2
    env, poly = make_set(m, D)
    n_segs, dts, _, _ = times_of_set()
    p, v, t, n_pts = point_sets()
    models = []
    for k in range(K):
        if not n_segs[k]:
            models.append(None)
            continue
        n = int(n_pts[k])
        lam, status = SM.build_lambda(p[:n, k], v[:n, k], t[:n, k], mode) if n <= 9 else (None, SM.BAD_POINTS)
        models.append(SM.with_Ts(lam, status, taus_of(dts[:, k], n_segs[k])))
    got = {r["status"] for r in models if r is not None}
    assert got == ({0, m.LAMBDA_BAD_POINTS, m.LAMBDA_NOT_POSITIVE} if mode == ROB else {0, m.LAMBDA_BAD_POINTS})
    assert max(r["lam"].n for r in models if r is not None and r["lam"] is not None) == 8
    pts = np.zeros((9, 3, K))
    pts[:, 0], pts[:, 1], pts[:, 2] = p, v, t
    rows = env.alloc_lambda_rows(K, WMAX)
    rows.fill(FILL)
    d_pts, d_n = m.DeviceArray(env, pts.nbytes), m.DeviceArray(env, K * 4)
    d_pts.upload(pts)
    d_n.upload(n_pts)
    poly.set_lambda_resident(rows, d_pts, n_pts=d_n, robust=mode == ROB)
    env.synchronize()
    check_build(rows.download(), models, n_segs, "set_lambda_device", (FILL, FILL_I32, FILL_F64))
    h = poly.set_lambda(p, v, t, n_pts=n_pts, robust=mode == ROB)
    check_build(h, models, n_segs, "set_lambda", (0, 0, 0.0))
    for b in (rows, d_pts, d_n, poly):
        b.free()
    env.close()


def device_times(mode):
    """[K][9] per-trajectory real times.  ROBUST: below 0, 0, six inside in ascending order, past the total.  REFERENCE:
    total (i + 1/2) / 9."""
    models = scale_models(mode)
    rng = np.random.default_rng(5)
    times = np.zeros((K, N))
    for k, r in enumerate(models):
        if r is None or r["status"]:
            times[k] = np.linspace(0.0, 1.0, N)
            continue
        total = r["total"]
        if mode == ROB:
            times[k] = [-0.37, 0.0] + list(np.sort(rng.uniform(0, float(total), 5))) + [float(total), float(total) + 0.5]
        else:
            times[k] = [total * F((i + 0.5) / N) for i in range(N)]
    return times


@functools.lru_cache(maxsize=None)
def reference_roots():
    """Per problem and time of device_times(REF): (model tau, found, exact root next to it or None).  Once, shared."""
    models, times = scale_models(REF), device_times(REF)
    out = []
    for k, r in enumerate(models):
        if r is None or r["status"]:
            out.append(None)
            continue
        row = []
        for t in times[k]:
            tau, found, seg, _ = r["lam"].get_tau_reference(t, want_info=True)
            row.append((tau, found, SM.exact_tau(r["lam"].segs[seg], 0.0, t, bits=80, near=tau) if found else None))
        out.append(row)
    return out


def test_tau_robust(engine):
    m = engine
    env, poly = make_set(m, 2)
    n_segs, dts, ri, rf = times_of_set()
    models, times = scale_models(ROB), device_times(ROB)
    poly.scale(ri, rf, robust=True)
    got = poly.tau(times=times)
    worst = 0.0
    for k, r in enumerate(models):
        if r is None:
            assert not got["tau"][k].any() and not got["found"][k].any()  # a failed load keeps the caller's zeros
            continue
        if r["status"]:  # no Lambda: the identity
            same_bits(got["tau"][k], times[k], "tau of the unscaled problem %d" % k)
            assert (got["lambda"][k] == 1).all() and (got["lambda_dot"][k] == 0).all() and (got["found"][k] == 1).all()
            continue
        lam, total, T = r["lam"], r["total"], taus_of(dts[:, k], n_segs[k])[-1]
        tau = got["tau"][k]
        assert (got["found"][k] == 1).all()
        assert tau[0] == 0 and tau[1] == 0, k
        same_bits(tau[-2:], [T, T], "tau at and past the total of problem %d" % k)
        assert (np.diff(tau) >= 0).all(), (k, tau)
        for q in range(2, N - 2):
            res = abs(float(lam.getT(tau[q])) - times[k, q]) / (EPS * float(total))
            worst = max(worst, res)
            assert res <= FACTOR, "problem %d, time %d: |getT(tau) - t| = %.2f * 2^-52 * total" % (k, q, res)
        for q in range(N):
            _, l, ld = lam.clamp_eval(tau[q], total, T)
            same_bits([got["lambda"][k, q], got["lambda_dot"][k, q]], [l, ld], "lambda at the device's tau, problem %d time %d" % (k, q))
    print("ROBUST: worst |getT(tau) - t| / (2^-52 total) = %.3f" % worst)
    # the uniform form: i * (total / N), the last one the total itself
    u = poly.tau(N=N)
    for k, r in enumerate(models):
        if r is None or r["status"]:
            continue
        assert u["tau"][k, 0] == 0
        same_bits(u["tau"][k, N], taus_of(dts[:, k], n_segs[k])[-1], "the last uniform tau of problem %d" % k)
    poly.free()
    env.close()


def test_tau_reference(engine):
    m = engine
    env, poly = make_set(m, 2)
    n_segs, dts, ri, rf = times_of_set()
    models, times, roots = scale_models(REF), device_times(REF), reference_roots()
    poly.scale(ri, rf, robust=False)
    got = poly.tau(times=times)
    worst, left_out, cases = 0.0, 0, 0
    for k, r in enumerate(models):
        if r is None or r["status"]:
            continue
        lam, total, T = r["lam"], r["total"], taus_of(dts[:, k], n_segs[k])[-1]
        for q in range(N):
            m_tau, m_found, truth = roots[k][q]
            cases += 1
            if m_found and min(abs(float(m_tau)), abs(float(m_tau) - float(T))) <= 1e-9:
                left_out += 1
                continue
            assert bool(got["found"][k, q]) == m_found, (k, q, got["tau"][k, q], m_tau)
            if not m_found:
                assert got["tau"][k, q] == -1
            else:
                assert truth is not None
                e_dev, e_mod = SM.err(got["tau"][k, q], truth), SM.err(m_tau, truth)
                worst = max(worst, e_dev / max(e_mod, EPS * float(T)))
                assert e_dev <= FACTOR * max(e_mod, EPS * float(T)), (k, q, got["tau"][k, q], m_tau, e_dev, e_mod)
            _, l, ld = lam.clamp_eval(got["tau"][k, q], total, T)
            same_bits([got["lambda"][k, q], got["lambda_dot"][k, q]], [l, ld], "lambda at the device's tau, problem %d time %d" % (k, q))
    print("REFERENCE: worst e_dev / max(e_model, 2^-52 tf) = %.3f; %d of %d cases left out" % (worst, left_out, cases))
    assert left_out <= 0.02 * cases
    poly.free()
    env.close()


def model_samples(D, r, n_segs_k, dts_k, k, times, raw, form_command):
    """The model's rows at the device's own getTau values `raw` [count]."""
    coef = coeff_of_set(D)[:n_segs_k, :D, :, k]
    cyaw = coeff_of_set(D)[:n_segs_k, D, :, k]
    taus = taus_of(dts_k, n_segs_k)
    rows = np.zeros((4 * D + (3 if form_command else 1), len(times)))
    for i, t in enumerate(times):
        if r is None:  # no Lambda: tau = the time clamped to [0, T], lambda = 1
            tau, l, ld = min(max(F(t), F(0.0)), taus[-1]), F(1.0), F(0.0)
        else:
            tau, l, ld = r["lam"].clamp_eval(raw[i], r["total"], taus[-1])
        rows[:, i] = SM.sample_rows(coef, cyaw, taus, tau, l, ld, t, form_command)
    return rows


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [2, 3])
def test_sample_with_lambda(engine, D, mode):
    m = engine
    env, poly = make_set(m, D)
    n_segs, dts, ri, rf = times_of_set()
    models = scale_models(mode)
    times = device_times(mode)
    sentinel = -7.25e77
    before = {(form, "u"): poly.sample(N=N, form=form)["samples"] for form in (m.TRAJ_COMMAND, m.TRAJ_WAYPOINT)}
    before.update({(form, "q"): poly.sample(times=times, form=form)["samples"] for form in (m.TRAJ_COMMAND, m.TRAJ_WAYPOINT)})
    poly.scale(ri, rf, robust=mode == ROB)
    tau_u, tau_q = poly.tau(N=N), poly.tau(times=times)
    ends = poly.info(want_states=True)["seg_state"]
    for form in (m.TRAJ_COMMAND, m.TRAJ_WAYPOINT):
        rows = 4 * D + (3 if form == m.TRAJ_COMMAND else 1)
        for kind, tq, raw_all in (("u", None, tau_u["tau"]), ("q", times, tau_q["tau"])):
            out = np.full((4 * D + 3, K, N + 1 if tq is None else N), sentinel)
            got = poly.sample(N=N if tq is None else None, times=tq, form=form, out=out)["samples"]
            for k, r in enumerate(models):
                if r is None:
                    assert (got[:, k] == sentinel).all(), (form, kind, k)  # a failed load keeps the caller's bytes
                    continue
                if r["status"]:  # no Lambda for this problem: what it returned before
                    same_bits(got[:rows, k], before[(form, kind)][:rows, k], "unscaled problem %d (form %d, %s)" % (k, form, kind))
                    continue
                if tq is None:
                    step = r["total"] / F(N)
                    ts = [F(i) * step for i in range(N + 1)]
                    if mode == ROB:
                        ts[N] = r["total"]
                else:
                    ts = tq[k]
                want = model_samples(D, r, int(n_segs[k]), dts[:, k], k, ts, raw_all[k], form == m.TRAJ_COMMAND)
                same_rows(got[:rows, k], want, "samples of problem %d (form %d, %s)" % (k, form, kind))
                assert (got[rows:, k] == sentinel).all()
                if mode == ROB and tq is None and form == m.TRAJ_WAYPOINT:  # the last uniform sample is the END state
                    end = ends[:4 * D + 1, n_segs[k], k]
                    assert np.allclose(got[:4 * D + 1, k, N], end, rtol=0, atol=1e-9 * (1 + np.abs(end).max())), k
    # clear_lambda: exactly what the poly returned before it held one
    poly.clear_lambda()
    for form in (m.TRAJ_COMMAND, m.TRAJ_WAYPOINT):
        same_bits(poly.sample(N=N, form=form)["samples"], before[(form, "u")], "after clear_lambda (form %d)" % form)
        same_bits(poly.sample(times=times, form=form)["samples"], before[(form, "q")], "after clear_lambda (form %d, times)" % form)
    poly.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ scale_down
def down_truth(D, k, S, dts_k, mv, ma):
    """The exact max_l of problem k and the exact times of every extremum (with taus added), for the 8 x rule."""
    import mpmath as mp
    taus = taus_of(dts_k, S)
    best, roots, scale = mp.mpf(0), [], 0.0
    for s in range(S):
        for i in range(D):
            c = coeff_of_set(D)[s, i, :, k]
            for order, lim in ((1, mv), (2, ma)):
                if not lim > 0:
                    continue
                x = LM.truth_all(c, dts_k[s], order) / mp.mpf(lim)
                l = x if order == 1 else mp.sqrt(x)
                if l > best:
                    best, scale = l, LM.scale_of(c, dts_k[s], order) / lim
                roots += [float(taus[s]) + float(r) for r in LM.true_roots(c, order) if 0 < r < dts_k[s]]
    return best, roots, scale


@pytest.mark.parametrize("D", [2, 3])
def test_scale_down(engine, D):
    m = engine
    mv, ma = 6.0, 4.0  # about three quarters of the set break them
    env, poly = make_set(m, D, v_max=mv, a_max=ma)
    n_segs, dts, _, _ = times_of_set()
    coef = coeff_of_set(D)
    rows = env.alloc_lambda_rows(K, WMAX)
    rows.fill(FILL)
    poly.scale_down_resident(rows, ri=1.0, rf=1.0, robust=True)  # limits: the EnvMap's
    env.synchronize()
    d = rows.download()
    h = poly.scale_down(ri=1.0, rf=1.0, robust=True)
    n_scaled, worst = 0, 0.0
    for k in range(K):
        S = int(n_segs[k])
        if S == 0:
            assert d["scaled"][k] == FILL and d["status"][k] == FILL and h["scaled"][k] == 0
            continue
        taus = taus_of(dts[:, k], S)
        w = SM.scale_down([coef[s, :D, :, k] for s in range(S)], dts[:S, k], taus, mv, ma, 1.0, 1.0, ROB)
        assert d["scaled"][k] == w["scaled"] == h["scaled"][k], k
        if not w["scaled"]:
            same_bits([d["max_l"][k], d["total"][k]], [FILL_F64, FILL_F64], "rows of the unscaled problem %d" % k)
            assert d["n_lseg"][k] == FILL_I32 and h["n_lseg"][k] == 0
            continue
        n_scaled += 1
        truth, roots, scale = down_truth(D, k, S, dts[:S, k], mv, ma)
        e_dev, e_mod = LM.err(d["max_l"][k], truth), LM.err(w["max_l"], truth)
        worst = max(worst, e_dev / max(e_mod, EPS * scale))
        assert e_dev <= FACTOR * max(e_mod, EPS * scale), (k, d["max_l"][k], w["max_l"], float(truth))
        for key in ("t_lo", "t_hi"):
            ends = [float(x) for x in taus]
            if float(w[key]) in ends:  # a candidate at an end of a segment: IEEE arithmetic
                same_bits(d[key][k], w[key], "%s of problem %d" % (key, k))
                continue
            near = min(roots, key=lambda r: abs(r - float(w[key])))
            assert abs(d[key][k] - near) <= FACTOR * max(abs(float(w[key]) - near), EPS * float(taus[-1])), (k, key, d[key][k], w[key], near)
        for key in ("max_l", "t_lo", "t_hi", "total", "status", "n_lseg"):
            same_bits(np.float64(h[key][k]), np.float64(d[key][k]), "host and device form, %s of problem %d" % (key, k))
        # the Lambda is set_lambda's on the device's own points
        p = [F(1.0), d["max_l"][k]] + ([d["max_l"][k]] if d["t_hi"][k] > d["t_lo"][k] else []) + ([F(1.0)] if taus[-1] > d["t_hi"][k] else [])
        t = [F(0.0), d["t_lo"][k]] + ([d["t_hi"][k]] if d["t_hi"][k] > d["t_lo"][k] else []) + ([taus[-1]] if taus[-1] > d["t_hi"][k] else [])
        lam, status = SM.build_lambda(p, [F(0.0)] * len(p), t, ROB)
        assert d["status"][k] == status == 0 and d["n_lseg"][k] == lam.n
        same_bits(d["segs"][:lam.n, :, k], lam.segs, "segments of problem %d" % k)
        same_bits(d["total"][k], SM.with_Ts(lam, 0, taus)["total"], "total of problem %d" % k)
    print("scale_down: %d of %d scaled; worst e_dev / max(e_model, 2^-52 scale) of max_l = %.3f" % (n_scaled, K, worst))
    assert 10 <= n_scaled < (n_segs > 0).sum()

    # a uniform scaling (no ramps): every device sample is within the limits, and a set within them comes back unscaled
    h = poly.scale_down(ri=0.0, rf=0.0, robust=True)
    s = poly.sample(N=64)["samples"]
    top_v = top_a = 0.0
    for k in range(K):
        if not h["scaled"][k]:
            continue
        v, a = np.abs(s[D:2 * D, k]).max(), np.abs(s[2 * D:3 * D, k]).max()
        assert v <= mv * (1 + 4 * EPS) and a <= ma * (1 + 4 * EPS), (k, v, a)
        top_v, top_a = max(top_v, v / mv), max(top_a, a / ma)
    assert max(top_v, top_a) > 0.9  # the limit is met somewhere, not merely undercut
    again = poly.scale_down(v_max=1e3, a_max=1e3)
    assert not again["scaled"].any() and not again["n_lseg"].any()
    unscaled = poly.sample(N=N)["samples"]
    poly.clear_lambda()
    same_bits(unscaled, poly.sample(N=N)["samples"], "a set scale_down left alone samples as without a Lambda")
    rows.free()
    poly.free()
    env.close()


def test_errors_and_state(engine):
    m = engine
    L = m._abi.lib()
    env, poly = make_set(m, 2)
    n_segs, dts, ri, rf = times_of_set()
    env.setMap([-20.0, -20.0], [16, 16], np.zeros(256, np.int8), 2.5)
    lo, li = m._abi.LambdaOut(), m._abi.ScaleIn()
    li.ri = li.rf = 1.0
    # MPLX_ERR_STATE before any solve or load, and for tau without a Lambda
    empty = env.alloc_poly(4, 3)
    li.mode = m.SCALE_ROBUST
    assert L.mplx_poly_scale_device(empty._h, C.byref(li), C.byref(lo)) == m._abi.ERR_STATE
    assert L.mplx_poly_scale(empty._h, C.byref(li), C.byref(lo)) == m._abi.ERR_STATE
    di, do = m._abi.ScaleDownIn(), m._abi.ScaleDownOut()
    di.mode = m.SCALE_ROBUST
    assert L.mplx_poly_scale_down(empty._h, C.byref(di), C.byref(do)) == m._abi.ERR_STATE
    tt, to = m._abi.TrajTimes(), m._abi.TauOut()
    tt.n_uniform = 4
    assert L.mplx_poly_tau(poly._h, C.byref(tt), C.byref(to)) == m._abi.ERR_STATE
    empty.free()
    # MPLX_ERR_ARG
    assert L.mplx_poly_scale(None, C.byref(li), C.byref(lo)) == m._abi.ERR_ARG
    assert L.mplx_poly_scale(poly._h, None, C.byref(lo)) == m._abi.ERR_ARG
    assert L.mplx_poly_scale(poly._h, C.byref(li), None) == m._abi.ERR_ARG
    li.mode = 2
    assert L.mplx_poly_scale(poly._h, C.byref(li), C.byref(lo)) == m._abi.ERR_ARG
    li.mode = m.SCALE_ROBUST
    buf = np.zeros((WMAX, K))
    lo.Ts, lo.ts_stride = buf.ctypes.data, K - 1
    assert L.mplx_poly_scale(poly._h, C.byref(li), C.byref(lo)) == m._abi.ERR_ARG
    lo = m._abi.LambdaOut()
    pin = m._abi.LambdaIn()
    pin.mode = m.SCALE_ROBUST
    assert L.mplx_poly_set_lambda(poly._h, C.byref(pin), C.byref(lo)) == m._abi.ERR_ARG            # NULL pts
    pts = np.zeros((9, 3, K))
    pin.pts, pin.stride = pts.ctypes.data, K - 1
    assert L.mplx_poly_set_lambda(poly._h, C.byref(pin), C.byref(lo)) == m._abi.ERR_ARG            # stride < n_prob
    # traverse works on the unscaled poly, is refused on a scaled one, works again after clear_lambda
    before = poly.traverse()
    poly.scale(ri, rf)
    with pytest.raises(m._abi.MplxError) as e:
        poly.traverse()
    assert e.value.code == m._abi.ERR_STATE
    tt.n_uniform = 0  # bad times
    assert L.mplx_poly_tau(poly._h, C.byref(tt), C.byref(to)) == m._abi.ERR_ARG
    tt.n_uniform = 4
    to.tau, to.stride = buf.ctypes.data, 4  # stride < N + 1
    assert L.mplx_poly_tau(poly._h, C.byref(tt), C.byref(to)) == m._abi.ERR_ARG
    # a load of no problems is a no-op: the Lambda stays
    scaled = poly.sample(N=N)["samples"]
    pi, po = m._abi.PolyLoadIn(), m._abi.PolyLoadOut()
    pi.n_prob, pi.w_max, pi.control = 0, WMAX, JRKxYAW
    assert L.mplx_poly_load(poly._h, C.byref(pi), C.byref(po)) == m._abi.OK
    same_bits(poly.sample(N=N)["samples"], scaled, "samples after a load of no problems")
    poly.clear_lambda()
    # a scale_down (host form) that scales nothing leaves a plain poly: traverse is not refused
    poly.scale(ri, rf)
    assert not poly.scale_down(v_max=1e3, a_max=1e3)["scaled"].any()
    after = poly.traverse()
    assert _tau_state(m, poly) == m._abi.ERR_STATE
    assert np.array_equal(before["n_samples"], after["n_samples"])
    same_bits(before["cost"], after["cost"], "traverse after clear_lambda")
    plain = poly.sample(N=N)["samples"]
    assert (bits_differ(plain, scaled)).any()
    # a new load into the poly clears the Lambda
    poly.scale(ri, rf)
    c = coeff_of_set(2)
    d_c, d_dt, d_n = m.DeviceArray(env, c.nbytes), m.DeviceArray(env, dts.nbytes), m.DeviceArray(env, K * 4)
    d_c.upload(c)
    d_dt.upload(dts)
    d_n.upload(n_segs)
    env.load_traj_resident(poly, d_c, d_dt, K, WMAX, n_segs=d_n, control=JRKxYAW)
    env.synchronize()
    same_bits(poly.sample(N=N)["samples"], plain, "samples after a new load")
    assert L.mplx_poly_tau(poly._h, C.byref(tt), C.byref(m._abi.TauOut())) == m._abi.ERR_STATE
    poly.traverse()
    for b in (d_c, d_dt, d_n, poly):
        b.free()
    env.close()


def same_rows(got, want, what):
    """Bit for bit, but a NaN is a NaN: the device's and the host's default NaNs differ in sign."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: the NaNs sit elsewhere" % what
    same_bits(np.where(np.isnan(got), 0.0, got), np.where(np.isnan(want), 0.0, want), what)


def bits_differ(a, b):
    return np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)


def _tau_state(m, poly):
    """The return code of mplx_poly_tau for four uniform samples, outputs not asked for."""
    tt = m._abi.TrajTimes()
    tt.n_uniform = 4
    return m._abi.lib().mplx_poly_tau(poly._h, C.byref(tt), C.byref(m._abi.TauOut()))


def test_a_new_solve_clears_the_lambda(engine):
    """mplx_solve_device into a poly that holds a Lambda: the samples are those of the same solve into a fresh poly, bit
    for bit, and the poly holds no Lambda (mplx_poly_tau: MPLX_ERR_STATE).  The stride changes with the solve (K = 70
    scaled problems, 37 solved ones), so a Lambda table that survived would be read with the wrong stride."""
    m = engine
    from test_gpu_solve import problems
    env, poly = make_set(m, 2)
    n_segs, dts, ri, rf = times_of_set()
    wp, n_wp, sdts, _ = problems(2)
    Ks, W = 37, wp.shape[1]
    assert W <= WMAX + 1
    wp, n_wp, sdts = np.ascontiguousarray(wp[:, :, :Ks]), np.ascontiguousarray(n_wp[:Ks]), np.ascontiguousarray(sdts[:, :Ks])
    d_wp, d_n, d_dt = m.DeviceArray(env, wp.nbytes), m.DeviceArray(env, Ks * 4), m.DeviceArray(env, sdts.nbytes)
    d_wp.upload(wp)
    d_n.upload(n_wp)
    d_dt.upload(sdts)
    big = env.alloc_poly(K, W)          # the one that gets scaled first
    fresh = env.alloc_poly(K, W)
    c = np.zeros((W - 1, 3, 6, K))
    c[:WMAX - 1] = coeff_of_set(2)
    dd = np.ones((W - 1, K))
    dd[:WMAX - 1] = dts
    d_c, d_d, d_s = m.DeviceArray(env, c.nbytes), m.DeviceArray(env, dd.nbytes), m.DeviceArray(env, K * 4)
    d_c.upload(c)
    d_d.upload(dd)
    d_s.upload(n_segs)
    env.load_traj_resident(big, d_c, d_d, K, W, n_segs=d_s, control=JRKxYAW)
    big.scale(ri, rf)
    assert _tau_state(m, big) == m._abi.OK
    scaled = big.sample(N=N)["samples"]
    poly.scale(ri, rf)
    same_bits(scaled, poly.sample(N=N)["samples"], "the scaled set in the larger poly")
    for p in (big, fresh):
        env.solve_traj_resident(p, d_wp, Ks, W, n_wp=d_n, dts=d_dt, control=m.JRK)
    env.synchronize()
    assert _tau_state(m, big) == m._abi.ERR_STATE
    for form in (m.TRAJ_COMMAND, m.TRAJ_WAYPOINT):
        a, b = big.sample(N=N, form=form), fresh.sample(N=N, form=form)
        same_bits(a["samples"], b["samples"], "samples after a solve into a scaled poly (form %d)" % form)
        assert np.array_equal(a["status"], b["status"]) and (a["status"] == 0).sum() > 20
    same_bits(big.info()["total_time"], fresh.info()["total_time"], "total time after a solve into a scaled poly")
    for b in (d_wp, d_n, d_dt, d_c, d_d, d_s, big, fresh, poly):
        b.free()
    env.close()


def test_the_gather_load_neither_keeps_nor_copies_a_lambda(engine):
    """The gather form of mplx_poly_load: into a scaled poly it clears the Lambda; from a scaled source it does not copy
    the source's.  Both results are the gather from a plain source into a fresh poly, bit for bit."""
    m = engine
    L = m._abi.lib()
    env, src = make_set(m, 2)
    n_segs, dts, ri, rf = times_of_set()
    Q, W = 40, 4
    rng = np.random.default_rng(9)
    good = np.flatnonzero(n_segs > 0)
    idx = np.full((W - 1, Q), -1, np.int32)
    for q in range(Q):
        n = 1 + q % (W - 1)
        idx[:n, q] = rng.choice(good, n)
    d_idx = m.DeviceArray(env, idx.nbytes)
    d_idx.upload(idx)

    def gather(target):
        i, o = m._abi.PolyLoadIn(), m._abi.PolyLoadOut()
        i.n_prob, i.w_max, i.control = Q, W, JRKxYAW
        i.src, i.src_index, i.index_stride = src._h, d_idx.ptr, Q
        m._abi.check(env._ctx, L.mplx_poly_load_device(target._h, C.byref(i), C.byref(o)))
        target.n, target.n_wmax, target._host, target._lambda = Q, W, None, None
        env.synchronize()

    plain, into_scaled, from_scaled = env.alloc_poly(K, WMAX), env.alloc_poly(K, WMAX), env.alloc_poly(K, WMAX)
    gather(plain)
    want = plain.sample(N=N)["samples"]
    assert np.isfinite(want[0]).all()
    # a target that holds a Lambda (of K problems: another stride)
    c, d_n = coeff_of_set(2), m.DeviceArray(env, K * 4)
    d_c, d_d = m.DeviceArray(env, c.nbytes), m.DeviceArray(env, dts.nbytes)
    d_c.upload(c)
    d_d.upload(dts)
    d_n.upload(n_segs)
    env.load_traj_resident(into_scaled, d_c, d_d, K, WMAX, n_segs=d_n, control=JRKxYAW)
    into_scaled.scale(ri, rf)
    gather(into_scaled)
    assert _tau_state(m, into_scaled) == m._abi.ERR_STATE
    same_bits(into_scaled.sample(N=N)["samples"], want, "a gather into a scaled poly")
    # a source that holds one
    src.scale(ri, rf)
    gather(from_scaled)
    assert _tau_state(m, src) == m._abi.OK and _tau_state(m, from_scaled) == m._abi.ERR_STATE
    same_bits(from_scaled.sample(N=N)["samples"], want, "a gather from a scaled poly")
    for b in (d_idx, d_c, d_d, d_n, plain, into_scaled, from_scaled, src):
        b.free()
    env.close()


@pytest.mark.parametrize("mode", MODES)
def test_tau_device_form_agrees_with_the_host_form(engine, mode):
    """mplx_poly_tau_device on rows filled with a pattern, with a row stride above the sample count: what the host form
    returns, bit for bit; the rows of failed loads and the entries past the count keep the pattern."""
    m = engine
    env, poly = make_set(m, 2)
    n_segs, dts, ri, rf = times_of_set()
    times = device_times(mode)
    poly.scale(ri, rf, robust=mode == ROB)
    stride = N + 3
    rows = env.alloc_lambda_rows(K, WMAX, stride)
    d_t = m.DeviceArray(env, times.nbytes)
    d_t.upload(times)
    for kind, host in (("times", poly.tau(times=times)), ("uniform", poly.tau(N=N))):
        count = N if kind == "times" else N + 1
        rows.fill(FILL)
        if kind == "times":
            poly.tau_resident(rows, times=d_t, n_times=N, time_stride=N)
        else:
            poly.tau_resident(rows, N=N)
        env.synchronize()
        d = rows.download()
        for k in range(K):
            for key in ("tau", "lambda", "lambda_dot"):
                if n_segs[k] == 0:
                    same_bits(d[key][k], np.full(stride, FILL_F64), "%s of the failed load %d (%s)" % (key, k, kind))
                    continue
                same_rows(d[key][k, :count], host[key][k], "%s of problem %d (%s)" % (key, k, kind))
                same_bits(d[key][k, count:], np.full(stride - count, FILL_F64), "%s past the count, problem %d (%s)" % (key, k, kind))
            want = host["found"][k] if n_segs[k] else np.full(count, FILL, np.uint8)
            assert np.array_equal(d["found"][k, :count], want) and (d["found"][k, count:] == FILL).all(), (k, kind)
    # the device form's own checks: a stride below the count, no Lambda
    tt, to = m._abi.TrajTimes(), rows.c_tau()
    tt.n_uniform, to.stride = N, N
    assert m._abi.lib().mplx_poly_tau_device(poly._h, C.byref(tt), C.byref(to)) == m._abi.ERR_ARG
    poly.clear_lambda()
    to.stride = stride
    assert m._abi.lib().mplx_poly_tau_device(poly._h, C.byref(tt), C.byref(to)) == m._abi.ERR_STATE
    for b in (rows, d_t, poly):
        b.free()
    env.close()
