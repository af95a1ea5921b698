"""Caller-given trajectories and dynamic limits on the device (include/mplx_limits.h, csrc/limits_kernel.hip) against
tests/limits_model.py.

Bit for bit: everything a load writes, every info / sample / traverse of a loaded set against the solved set it was
loaded from, and the limits wherever the result does not pass through cbrt / acos / cos (solver outputs with smoothing
order 0 and 1, crafted segments).  Held to a bound: the limits of full quintics, where the device library's cbrt / acos /
cos differ from the host's.  Per value, with truth = the exact maximum (limits_model.truth_*), e_ref = |model - truth|,
e_dev = |device - truth| and scale = the sum of the absolute terms of the polynomial at T,

    e_dev <= 8 * max(e_ref, 2^-52 * scale)

-- the convention of tests/test_gpu_solve.py for results of a different but equivalent evaluation.  A REFERENCE value
would be left out where a root the model computed lies within 2^-30 T of 0 or T (acceptance could flip between the two
libraries); on these inputs there is none.  The worst ratio per mode is printed (pytest -s) and recorded in DESIGN.md 4.16.

One thing a loaded set cannot share with the solved one: its waypoints (info's seg_state).  A solve stores the waypoint
rows it was given, free derivatives included; a load evaluates them from the segments.  They are compared with the
model's evaluation bit for bit, and with the solved set's positions where a position is a stored coefficient.

Shapes: K = 67 (a wave and three lanes), D in {2, 3}, 2 .. 7 waypoints; the 400 quintics are K larger than a workgroup."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import limits_model as LM
import traj_model as TM
from test_gpu_solve import CONTROLS, K, SENTINEL, WMAX, make_env, model_set, same_bits, solve_set, traverse_world
from test_limits_model import IEEE_ONLY

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
FACTOR = 8.0
REF, ALL = LM.REFERENCE, LM.ALL_ROOTS
KEYS = ("max_vel", "max_acc", "max_jrk")


def coefs_of(poly, k):
    """Per segment [D][6] and the durations of problem k, from what the device holds."""
    S = int(poly.n_segs[k])
    seg = poly.segments()
    D = seg.shape[1] - 1
    return [seg[s, :D, :, k] for s in range(S)], poly.dts()[:S, k]


def model_limits(poly, control, mv, ma, mj, mode):
    out = []
    for k in range(poly.n):
        if poly.n_segs[k] == 0:
            out.append(None)
            continue
        cs, dts = coefs_of(poly, k)
        out.append(LM.traj_limits(cs, dts, control, mv, ma, mj, mode))
    return out


def check_exact(got, want, what):
    """Device limits against the model's, bit for bit; a failed problem keeps the zeros / -1 of PolyTrajSet.limits."""
    for k, w in enumerate(want):
        if w is None:
            assert not any(got[key][:, k].any() for key in KEYS) and got["valid"][k] == 0 and got["first_bad"][k] == -1, (what, k)
            continue
        for key in KEYS:
            same_bits(got[key][:, k], w[key], "%s: %s of problem %d" % (what, key, k))
        assert (got["exceed"][k], got["valid"][k], got["first_bad"][k]) == (w["exceed"], w["valid"], w["first_bad"]), (what, k)


@pytest.mark.parametrize("D,so", [(D, so) for D in (2, 3) for so in (0, 1, 2)], ids=lambda x: str(x))
def test_load_equals_the_solved_set(engine, D, so):
    m = engine
    env = make_env(m, D)
    solved = solve_set(env, D, so, "given")
    seg, dts = solved.segments(), solved.dts()
    loaded = env.load_traj(seg, dts, n_segs=solved.n_segs, control=CONTROLS[so])
    assert loaded.n == K and np.array_equal(loaded.status, solved.status) and np.array_equal(loaded.n_segs, solved.n_segs)
    assert (loaded.status[solved.n_segs == 0] == m.SOLVE_EMPTY).all() and (solved.n_segs == 0).sum() > 5
    same_bits(loaded.total_time, solved.total_time, "total_time")
    same_bits(loaded.taus(), solved.taus(), "taus")
    same_bits(loaded.segments(), seg, "segments")
    a, b = loaded.info(want_states=True), solved.info(want_states=True)
    for key in ("status", "n_segs"):
        assert np.array_equal(a[key], b[key]), key
    same_bits(a["total_time"], b["total_time"], "info total_time")
    same_bits(a["effort"], b["effort"], "efforts")
    trajs = model_set(solved, D, so)
    rng = np.random.default_rng(3)
    times = np.zeros((K, 5))
    for k, tr in enumerate(trajs):
        if tr is None:
            assert not a["seg_state"][:, :, k].any()
            continue
        # waypoint s: segment s at 0.0, the last one: the last segment at its duration; t = taus[s]
        want = np.zeros((4 * D + 2, tr.S + 1))
        for w in range(tr.S + 1):
            s, t = min(w, tr.S - 1), np.float64(0.0 if w < tr.S else tr.dts[-1])
            for i in range(D):
                c = tr.coef[s][i]
                want[i, w], want[D + i, w], want[2 * D + i, w], want[3 * D + i, w] = (f(c, t) for f in (TM.poly_p, TM.poly_v, TM.poly_a, TM.poly_j))
            want[4 * D, w] = TM.normalize_angle(TM.poly_p(tr.coef_yaw[s], t))
            want[4 * D + 1, w] = tr.taus[w]
        same_bits(a["seg_state"][:, :tr.S + 1, k], want, "waypoints of problem %d" % k)
        same_bits(a["seg_state"][:D, :tr.S, k], b["seg_state"][:D, :tr.S, k], "positions of problem %d" % k)
        times[k] = [0.0, float(tr.taus[1]), tr.T, tr.T + 0.5] + [float(rng.uniform(0, tr.T))]
    for form in (m.TRAJ_COMMAND, m.TRAJ_WAYPOINT):
        for N, tq in ((23, None), (None, times)):
            x = loaded.sample(N=N, times=tq, form=form, out=np.full((4 * D + 3, K, 24 if N else 5), SENTINEL))
            y = solved.sample(N=N, times=tq, form=form, out=np.full((4 * D + 3, K, 24 if N else 5), SENTINEL))
            same_bits(x["samples"], y["samples"], "samples (form %d, N %r)" % (form, N))
            assert np.array_equal(x["status"], y["status"])
    for p in (loaded, solved):
        p.free()
    env.close()


def test_load_traverses_as_the_solved_set(engine):
    m = engine
    md, org, res = ([40, 33], [-1.5, 0.7], 0.25)
    grid, pot, wp, n_wp = traverse_world()
    env = make_env(m, 2, control=m.JRK)
    env.setMap(org, md, grid, res)
    env.set_potential_weight(0.1)
    env.set_gradient_weight(0.25)
    env.set_potential_map(pot)
    solved = env.solve_traj(wp, n_wp=n_wp, v=0.9, control=m.JRK)
    loaded = env.load_traj(solved.segments(), solved.dts(), n_segs=solved.n_segs, control=m.JRK)
    for lanes in (0, 4, 64):
        a, b = loaded.traverse(lanes=lanes), solved.traverse(lanes=lanes)
        for key in ("status", "n_samples", "n_cells", "stop_sample"):
            assert np.array_equal(a[key], b[key]), (lanes, key)
        same_bits(a["cost"], b["cost"], "cost (lanes %d)" % lanes)
    assert np.isfinite(b["cost"]).sum() > 5 and np.isinf(b["cost"]).sum() >= 3
    loaded.free()
    solved.free()
    env.close()


def _raw_load(m, env, poly, device, coeff, dts, n_segs, control, stride, w_max):
    """mplx_poly_load / _device with every stride = `stride` > K and sentinel-filled outputs; returns the outputs."""
    A, L = m._abi, m._abi.lib()
    Kp = coeff.shape[-1]
    host = {"status": np.full(stride, 0x5A, np.uint8), "n_segs": np.full(stride, -77, np.int32),
            "total_time": np.full(stride, SENTINEL), "taus": np.full((w_max, stride), SENTINEL)}
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, np.zeros(a.shape[:-1] + (stride - Kp,), a.dtype)], axis=-1))
    ins = {"coeff": pad(coeff), "dts": pad(dts), "n_segs": pad(n_segs)}
    i, o = A.PolyLoadIn(), A.PolyLoadOut()
    i.n_prob, i.w_max, i.control, i.dt_stride, i.coeff_stride, o.taus_stride = Kp, w_max, control, stride, stride, stride
    if device:
        bufs = []
        for struct, arrays in ((i, ins), (o, host)):  # (both have an n_segs: the input and the output)
            for key, a in arrays.items():
                b = m.DeviceArray(env, a.nbytes)
                b.upload(a)
                bufs.append((struct is o, key, b))
                setattr(struct, key, b.ptr)
        A.check(env._ctx, L.mplx_poly_load_device(poly._h, C.byref(i), C.byref(o)))
        env.synchronize()
        for is_out, key, b in bufs:
            if is_out:
                host[key] = b.download(host[key].dtype, host[key].shape)
            b.free()
    else:
        for key, a in ins.items():
            setattr(i, key, a.ctypes.data)
        for key, a in host.items():
            setattr(o, key, a.ctypes.data)
        A.check(env._ctx, L.mplx_poly_load(poly._h, C.byref(i), C.byref(o)))
    return host


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_load_statuses_and_untouched_memory(engine, device):
    """EMPTY for n_segs 0 and below, BAD_TIME for dt = 0, NaN, inf and a negative one -- also in a later segment --, n_segs
    above w_max - 1 counts as w_max - 1, mixed n_segs in one call; a failed problem writes its status only, taus rows past
    S_k and entries past K keep the sentinel; limits skip the failed problems."""
    m, D, w_max, Kp, stride = engine, 2, 4, 9, 12
    rng = np.random.default_rng(8)
    coeff = np.round(rng.uniform(-1, 1, (w_max - 1, D + 1, 6, Kp)), 3)
    coeff[:, :, :2, :] = 0.0  # (c0 = c1 = 0: the limits below are IEEE only)
    dts = np.round(rng.uniform(0.4, 1.5, (w_max - 1, Kp)), 2)
    n_segs = np.array([3, 0, 2, 3, 3, 1, 9, -2, 3], np.int32)
    dts[0, 2], dts[2, 3], dts[1, 4], dts[1, 8] = 0.0, np.nan, -0.5, np.inf
    dts[1, 5] = np.nan  # past S_5 = 1: not looked at
    EM, BT = m.SOLVE_EMPTY, m.SOLVE_BAD_TIME
    want = [0, EM, BT, BT, BT, 0, 0, EM, BT]
    S_of = [3, 0, 0, 0, 0, 1, 3, 0, 0]
    env = make_env(m, D)
    poly = env.alloc_poly(Kp, w_max)
    h = _raw_load(m, env, poly, device, coeff, dts, n_segs, m.ACC, stride, w_max)
    assert h["status"][:Kp].tolist() == want and (h["status"][Kp:] == 0x5A).all()
    for k in range(stride):
        S = S_of[k] if k < Kp else 0
        assert h["n_segs"][k] == (S if S else -77), k
        assert (h["total_time"][k] == SENTINEL) == (S == 0), k
        col = h["taus"][:, k]
        rows = S + 1 if S else 0
        assert not (col[:rows] == SENTINEL).any() and (col[rows:] == SENTINEL).all(), k
        if S:
            taus = np.concatenate([[0.0], np.cumsum(dts[:S, k])])  # (np.cumsum adds sequentially)
            same_bits(col[:rows], taus, "taus of problem %d" % k)
            assert h["total_time"][k] == taus[-1]
    poly.n, poly.n_wmax = Kp, w_max  # (the raw call went round the Python bookkeeping)
    out = {key: np.full((D, Kp), SENTINEL) for key in KEYS}
    out.update(exceed=np.full(Kp, 0x5A, np.uint8), valid=np.full(Kp, 0x5A, np.uint8), first_bad=np.full(Kp, -77, np.int32))
    o, i = m._abi.LimitsOut(), m._abi.LimitsIn()
    for key in out:
        setattr(o, key, out[key].ctypes.data)
    o.max_stride, i.mv, i.mode = Kp, 0.5, REF
    m._abi.check(env._ctx, m._abi.lib().mplx_poly_limits(poly._h, C.byref(i), C.byref(o)))
    for k in range(Kp):
        if S_of[k] == 0:
            assert (out["max_vel"][:, k] == SENTINEL).all() and out["valid"][k] == 0x5A and out["first_bad"][k] == -77, k
            continue
        w = LM.traj_limits([coeff[s, :D, :, k] for s in range(S_of[k])], dts[:S_of[k], k], m.ACC, 0.5, 0, 0, REF)
        for key in KEYS:
            same_bits(out[key][:, k], w[key], "%s of problem %d" % (key, k))
        assert (out["exceed"][k], out["valid"][k], out["first_bad"][k]) == (w["exceed"], w["valid"], w["first_bad"]), k
    poly.free()
    env.close()


@pytest.mark.parametrize("D,so", [(2, 0), (3, 0), (2, 1), (3, 1)], ids=lambda x: str(x))
@pytest.mark.parametrize("mode", [REF, ALL], ids=["reference", "all_roots"])
def test_limits_of_solver_outputs_ieee_only(engine, D, so, mode):
    """Smoothing order 0 and 1: c0 = c1 = 0, the root finder stays in its linear and quadratic branches."""
    m = engine
    env = make_env(m, D)
    poly = solve_set(env, D, so, "given")
    free = model_limits(poly, CONTROLS[so], 0, 0, 0, mode)
    tops = np.array([[w[key].max() for key in KEYS] for w in free if w is not None])
    mv, ma, mj = (float(np.median(tops[:, q])) for q in range(3))  # about half of the problems exceed each limit
    for lim in ((0.0, 0.0, 0.0), (mv, ma, mj), (-1.0, ma, 0.0)):
        got = poly.limits(*lim, all_roots=mode == ALL)
        check_exact(got, model_limits(poly, CONTROLS[so], *lim, mode), "limits %r" % (lim,))
    valid = poly.limits(mv, ma, mj, all_roots=mode == ALL)["valid"][poly.n_segs > 0]
    if so == 1:
        assert 10 < valid.sum() < len(valid) - 10  # an ACC set: the velocity decides
    else:
        assert valid.all()  # a VEL set is always valid
    poly.free()
    env.close()


def crafted_set(D):
    """The IEEE-only quirk cases of tests/test_limits_model.py as single-segment problems, the case on axis D - 1, plus a
    three-segment problem chaining the ones with c0 == 0: coeff [3][D + 1][6][K], dts [3][K], n_segs [K]."""
    Kc = len(IEEE_ONLY) + 1
    coeff, dts, n_segs = np.zeros((3, D + 1, 6, Kc)), np.ones((3, Kc)), np.ones(Kc, np.int32)
    for k, (_, c, T, _, _, _) in enumerate(IEEE_ONLY):
        coeff[0, D - 1, :, k], dts[0, k] = c, T
        coeff[0, 0, :, k] = [0, 0, 0.5, -0.25, 0.125, 1.0]
    chain = [c for c in IEEE_ONLY if c[1][0] == 0][:3]
    for s, (_, c, T, _, _, _) in enumerate(chain):
        coeff[s, 0, :, Kc - 1], dts[s, Kc - 1] = c, T
    n_segs[Kc - 1] = 3
    return coeff, dts, n_segs


@pytest.mark.parametrize("D", [2, 3])
def test_limits_of_crafted_segments(engine, D):
    """Every quirk that does not use the cubic branch, with the expected values of the CPU test: bit for bit, both modes.
    A case with c0 != 0 is about one order; its other orders go through the cubic and are not compared here."""
    m = engine
    coeff, dts, n_segs = crafted_set(D)
    env = make_env(m, D)
    poly = env.load_traj(coeff, dts, n_segs=n_segs, control=m.SNP)
    assert not poly.status.any()
    for mode in (REF, ALL):
        got = poly.limits(0, 0, 0, all_roots=mode == ALL)
        for k, (name, c, T, order, want_ref, want_all) in enumerate(IEEE_ONLY):
            same_bits(got[KEYS[order - 1]][D - 1, k:k + 1], [want_ref if mode == REF else want_all], name)
            if c[0] == 0:
                w = LM.traj_limits([coeff[0, :D, :, k]], dts[:1, k], m.SNP, 0, 0, 0, mode)
                for key in KEYS:
                    same_bits(got[key][:, k], w[key], "%s: %s" % (name, key))
        k = len(IEEE_ONLY)
        lim = (2.1, 3.6, 0.0)
        got = poly.limits(*lim, all_roots=mode == ALL)
        w = LM.traj_limits([coeff[s, :D, :, k] for s in range(3)], dts[:, k], m.SNP, *lim, mode)
        for key in KEYS:
            same_bits(got[key][:, k], w[key], "chain: %s" % key)
        assert (got["exceed"][k], got["valid"][k], got["first_bad"][k]) == (w["exceed"], w["valid"], w["first_bad"])
    poly.free()
    env.close()


def check_bound(dev, model, truth, scale, what):
    e_ref, e_dev = LM.err(model, truth), LM.err(dev, truth)
    floor = max(e_ref, EPS * scale)
    assert e_dev <= FACTOR * floor, "%s: device %r, model %r: e_dev %.3g, e_ref %.3g, scale %.3g: ratio %.2f > %g" % (
        what, dev, model, e_dev, e_ref, scale, e_dev / floor, FACTOR)
    return e_dev / floor


@pytest.mark.parametrize("D", [2, 3])
def test_limits_of_quintics_cubic_branch(engine, D):
    """The 400 quintics as single-segment problems (K larger than a workgroup): quintic k on axis 0, quintic k + 1 on
    the last axis (for the lanes' company: a segment has one duration, axis 0 is the one compared)."""
    m = engine
    coef, Ts = LM.quintics()
    ref = LM.quintic_reference()
    n = LM.N_QUINTICS
    coeff = np.zeros((1, D + 1, 6, n))
    coeff[0, 0], coeff[0, D - 1] = coef.T, np.roll(coef, -1, axis=0).T
    env = make_env(m, D)
    poly = env.load_traj(coeff, Ts[None, :], control=m.SNP)
    assert not poly.status.any()
    for mode in (REF, ALL):
        got = poly.limits(0, 0, 0, all_roots=mode == ALL)
        worst, left_out = 0.0, 0
        for k in range(n):
            for order in (1, 2, 3):
                r = ref[k][(mode, order)]
                if mode == REF and r["near"]:
                    left_out += 1
                    continue
                worst = max(worst, check_bound(got[KEYS[order - 1]][0, k], r["model"], r["truth"], r["scale"],
                                               "quintic %d, order %d, mode %d" % (k, order, mode)))
        assert left_out <= 0.02 * 3 * n
        print("quintics, D = %d, mode %d: worst e_dev / max(e_ref, eps scale) = %.3f, left out %d" % (D, mode, worst, left_out))
    poly.free()
    env.close()


@functools.lru_cache(maxsize=None)
def _truth_of_segment(c, T, order, mode):
    c = np.array(c)
    m, roots, ts = LM.axis_max(c, T, order, mode, want_roots=True)
    near = any(abs(r) <= 2.0 ** -30 * T or abs(r - T) <= 2.0 ** -30 * T for r in roots if np.isfinite(r))
    truth = LM.truth_reference(c, T, order, ts) if mode == REF else LM.truth_all(c, T, order)
    return truth, LM.scale_of(c, T, order), near


def test_limits_of_a_jerk_solve_and_decisions_with_margin(engine):
    """A smoothing order 2 solver set (D = 2): the maxima within the bound, then for every problem and each of vel / acc /
    jrk the limit at the model maximum x (1 + 2^-20) and x (1 - 2^-20), ten orders of magnitude outside the bound: exceed
    shows the right bit, valid follows the control (a JRK set ignores mj), first_bad is the model's segment."""
    m, D = engine, 2
    env = make_env(m, D)
    poly = solve_set(env, D, 2, "given")
    live = [k for k in range(K) if poly.n_segs[k] > 0]
    for mode in (REF, ALL):
        got = poly.limits(0, 0, 0, all_roots=mode == ALL)
        model = model_limits(poly, m.JRK, 0, 0, 0, mode)
        worst, left_out, total = 0.0, 0, 0
        for k in live[::3]:  # (the exact roots are the slow part; the decisions below run on every problem)
            cs, dts = coefs_of(poly, k)
            for q in range(3):
                for i in range(D):
                    parts = [_truth_of_segment(tuple(c[i]), float(t), q + 1, mode) for c, t in zip(cs, dts)]
                    total += 1
                    if mode == REF and any(p[2] for p in parts):
                        left_out += 1
                        continue
                    worst = max(worst, check_bound(got[KEYS[q]][i, k], model[k][KEYS[q]][i], max(p[0] for p in parts),
                                                   max(p[1] for p in parts), "problem %d, %s[%d], mode %d" % (k, KEYS[q], i, mode)))
        assert left_out <= 0.02 * total
        print("so = 2 solve, mode %d: worst e_dev / max(e_ref, eps scale) = %.3f, left out %d of %d" % (mode, worst, left_out, total))
    model = model_limits(poly, m.JRK, 0, 0, 0, REF)
    checked = LM.checks_of(m.JRK)
    for k in live:
        cs, dts = coefs_of(poly, k)
        for q in range(3):
            top = float(model[k][KEYS[q]].max())
            for f, over in ((1 + 2.0 ** -20, False), (1 - 2.0 ** -20, True)):
                lim = [0.0, 0.0, 0.0]
                lim[q] = top * f
                got = poly.limits(*lim)
                w = LM.traj_limits(cs, dts, m.JRK, *lim, REF)
                assert got["exceed"][k] == ((1 << q) if over else 0) == w["exceed"], (k, q, over)
                assert got["valid"][k] == (0 if over and checked[q] else 1) == w["valid"], (k, q, over)
                assert got["first_bad"][k] == w["first_bad"] and (w["first_bad"] >= 0) == (over and checked[q]), (k, q, over)
    poly.free()
    env.close()


def test_control_rules_with_margin(engine):
    """An ACC set ignores ma and mj, a VEL set is always valid, an SNP set checks all three: the same loaded segments
    under each control, limits at the ALL_ROOTS model maximum x (1 -+ 2^-20)."""
    m, D = engine, 3
    env = make_env(m, D)
    src = solve_set(env, D, 1, "given")
    seg, dts, n_segs = src.segments(), src.dts(), src.n_segs
    src.free()
    for control in (m.VEL, m.ACC, m.ACCxYAW, m.JRK, m.SNP, m.SNPxYAW):
        poly = env.load_traj(seg, dts, n_segs=n_segs, control=control)
        model = model_limits(poly, control, 0, 0, 0, ALL)
        checked = LM.checks_of(control)
        for k in range(0, K, 5):
            if model[k] is None:
                continue
            for q in range(3):
                top = float(model[k][KEYS[q]].max())
                if top == 0.0:  # (a cubic has no jerk term to exceed anything)
                    continue
                for f, over in ((1 + 2.0 ** -20, False), (1 - 2.0 ** -20, True)):
                    lim = [0.0, 0.0, 0.0]
                    lim[q] = top * f
                    got = poly.limits(*lim, all_roots=True)
                    assert got["exceed"][k] == ((1 << q) if over else 0), (control, k, q, over)
                    assert got["valid"][k] == (0 if over and checked[q] else 1), (control, k, q, over)
        poly.free()
    env.close()


def test_host_and_device_forms_agree(engine):
    m, D = engine, 3
    env = make_env(m, D)
    poly = solve_set(env, D, 2, "given")
    out = env.alloc_poly_limits(K)
    for mode in (REF, ALL):
        host = poly.limits(1.0, 1.5, 0.0, all_roots=mode == ALL)
        for b, fill in ((out.max_vel, 0.0), (out.max_acc, 0.0), (out.max_jrk, 0.0)):
            b.upload(np.full((D, K), fill))
        out.exceed.upload(np.zeros(K, np.uint8))
        out.valid.upload(np.zeros(K, np.uint8))
        out.first_bad.upload(np.full(K, -1, np.int32))
        poly.limits_resident(out, 1.0, 1.5, 0.0, all_roots=mode == ALL)
        env.synchronize()
        dev = out.download()
        for key in host:
            assert np.array_equal(np.asarray(host[key]).view(np.uint8), np.asarray(dev[key]).view(np.uint8)), (mode, key)
    # the resident load: the same table as the host-pointer load
    seg, dts, n_segs = poly.segments(), poly.dts(), poly.n_segs
    bufs = [m.DeviceArray(env, a.nbytes) for a in (seg, dts, n_segs)]
    for b, a in zip(bufs, (seg, dts, n_segs)):
        b.upload(a)
    res = env.alloc_poly(K, WMAX)
    env.load_traj_resident(res, bufs[0], bufs[1], K, WMAX, n_segs=bufs[2], control=m.JRK)
    with pytest.raises(RuntimeError, match="kept no output rows"):  # no `out`: nothing to read on the host
        res.status
    env.load_traj_resident(res, bufs[0], bufs[1], K, WMAX, n_segs=bufs[2], control=m.JRK, out=env.alloc_load_out(K, WMAX))
    assert np.array_equal(res.status, poly.status) and np.array_equal(res.n_segs, poly.n_segs)
    same_bits(res.total_time, poly.total_time, "total_time of the resident load")
    same_bits(res.taus(), poly.taus(), "taus of the resident load")
    with pytest.raises(RuntimeError, match="on the device only"):
        res.segments()
    a, b = res.limits(1.0, 1.5, 0.0, all_roots=True), poly.limits(1.0, 1.5, 0.0, all_roots=True)
    for key in a:
        assert np.array_equal(np.asarray(a[key]).view(np.uint8), np.asarray(b[key]).view(np.uint8)), key
    x, y = res.sample(N=9), poly.sample(N=9)
    same_bits(x["samples"], y["samples"], "samples of the resident load")
    for b_ in bufs:
        b_.free()
    out.free()
    res.free()
    poly.free()
    env.close()


def test_argument_errors(engine):
    m = engine
    A, L = m._abi, m._abi.lib()
    env = make_env(m, 2)
    poly = env.alloc_poly(4, 3)
    li, lo = A.LimitsIn(), A.LimitsOut()
    assert L.mplx_poly_limits(poly._h, C.byref(li), C.byref(lo)) == A.ERR_STATE  # nothing solved or loaded
    assert L.mplx_poly_limits_device(poly._h, C.byref(li), C.byref(lo)) == A.ERR_STATE
    coeff, dts = np.zeros((2, 3, 6, 4)), np.ones((2, 4))
    coeff[:, :2, 4, :] = 1.0

    def load(fn=None, **kw):
        i, o = A.PolyLoadIn(), A.PolyLoadOut()
        i.n_prob, i.w_max, i.control, i.dts, i.dt_stride, i.coeff, i.coeff_stride = 4, 3, 0x03, dts.ctypes.data, 4, coeff.ctypes.data, 4
        for key, val in kw.items():
            setattr(o if key.startswith("taus") else i, key, val)
        return (fn or L.mplx_poly_load)(poly._h, C.byref(i), C.byref(o))

    assert load(n_prob=0) == A.OK  # a no-op: still nothing loaded
    assert L.mplx_poly_limits(poly._h, C.byref(li), C.byref(lo)) == A.ERR_STATE
    assert load(coeff=None) == A.ERR_ARG and load(dts=None) == A.ERR_ARG
    assert load(dt_stride=3) == A.ERR_ARG and load(coeff_stride=3) == A.ERR_ARG
    taus = np.zeros((3, 4))
    assert load(taus=taus.ctypes.data, taus_stride=3) == A.ERR_ARG and load(taus=taus.ctypes.data, taus_stride=4) == A.OK
    assert load(w_max=1) == A.ERR_ARG and load(w_max=4) == A.ERR_ARG and load(n_prob=5, dt_stride=5, coeff_stride=5) == A.ERR_ARG
    assert load(control=0x05) == A.ERR_ARG and load(control=0x2F) == A.ERR_ARG and load(control=0x1F) == A.OK
    assert load(fn=L.mplx_poly_load_device, control=0x05) == A.ERR_ARG
    assert L.mplx_poly_load(poly._h, None, None) == A.ERR_ARG and L.mplx_poly_load(None, None, None) == A.ERR_ARG
    assert load() == A.OK
    assert L.mplx_poly_limits(poly._h, None, C.byref(lo)) == A.ERR_ARG and L.mplx_poly_limits(poly._h, C.byref(li), None) == A.ERR_ARG
    assert L.mplx_poly_limits(None, C.byref(li), C.byref(lo)) == A.ERR_ARG
    li.mode = 2
    assert L.mplx_poly_limits(poly._h, C.byref(li), C.byref(lo)) == A.ERR_ARG and b"mode" in L.mplx_last_error(env._ctx)
    li.mode = 1
    assert L.mplx_poly_limits(poly._h, C.byref(li), C.byref(lo)) == A.OK  # every output is optional
    mx = np.zeros((2, 4))
    lo.max_acc, lo.max_stride = mx.ctypes.data, 3
    assert L.mplx_poly_limits(poly._h, C.byref(li), C.byref(lo)) == A.ERR_ARG
    lo.max_stride = 4
    assert L.mplx_poly_limits(poly._h, C.byref(li), C.byref(lo)) == A.OK and not mx.any()  # constant velocity 1
    poly.free()
    env.close()


def test_connect_and_pick_fastest(engine):
    """EnvMap.connect: K two-point primitives whose ends are the given states; pick_fastest: per query the fastest
    candidate that is solved, valid under all_roots=True and traverses free space."""
    m, D = engine, 2
    env = make_env(m, D, control=m.JRK)
    md, org, res = ([40, 33], [-1.5, 0.7], 0.25)
    env.setMap(org, md, np.zeros(md[0] * md[1], np.int8), res)
    rng = np.random.default_rng(12)
    Kc = 7
    a, b = np.zeros((10, Kc)), np.zeros((10, Kc))
    a[:2], b[:2] = rng.uniform(1.0, 4.0, (2, Kc)), rng.uniform(1.0, 4.0, (2, Kc))
    a[2:6], b[2:6] = rng.uniform(-0.5, 0.5, (4, Kc)), rng.uniform(-0.5, 0.5, (4, Kc))
    T = rng.uniform(1.0, 3.0, Kc)
    poly = env.connect(a, b, T, control=m.JRK)
    assert not poly.status.any() and (poly.n_segs == 1).all()
    s = poly.sample(times=np.stack([np.zeros(Kc), T], axis=1), form=m.TRAJ_WAYPOINT)["samples"]
    assert np.abs(s[:6, :, 0] - a[:6]).max() <= 1e-12 and np.abs(s[:6, :, 1] - b[:6]).max() <= 1e-9
    poly.free()
    # 3 queries x 4 speeds on straight 3-waypoint paths: the faster the candidate, the larger its peak velocity
    Q, vs = 3, [0.5, 1.0, 2.0, 4.0]
    wp = np.zeros((10, 3, Q * len(vs)))
    for vi in range(len(vs)):
        for q in range(Q):
            wp[0, :, vi * Q + q] = [1.0, 2.0 + 0.5 * q, 3.5 + q]
            wp[1, :, vi * Q + q] = 3.0
    cand = env.solve_traj(wp, v=np.repeat(vs, Q), control=m.JRK)
    lim = cand.limits(0, 0, 0, all_roots=True)
    peak = lim["max_vel"].max(axis=0).reshape(len(vs), Q)
    assert (np.diff(peak, axis=0) > 0).all()
    v_lim = float(peak[2].max()) * 1.001  # speeds 0.5 .. 2 pass for every query, 4 fails
    assert (peak[3] > v_lim).all()
    assert m.pick_fastest(cand, Q, vs, v_max=v_lim, a_max=0, j_max=0).tolist() == [2, 2, 2]
    assert m.pick_fastest(cand, Q, vs, v_max=float(peak[0].min()) * 0.5, a_max=0, j_max=0).tolist() == [-1, -1, -1]
    assert m.pick_fastest(cand, Q, vs, v_max=0, a_max=0, j_max=0).tolist() == [3, 3, 3]
    grid = np.zeros((md[1], md[0]), np.int8)
    grid[:, 21:25] = 100  # a wall across x in [3.75, 4.75): query 0 ends before it, queries 1 and 2 cross it
    env.setMap(org, md, grid.ravel(), res)
    assert m.pick_fastest(cand, Q, vs, v_max=0, a_max=0, j_max=0).tolist() == [3, -1, -1]
    cand.free()
    env.close()
