"""The trajectory solver on the device (include/mplx_solve.h, csrc/solve_kernel.hip, the POLY instantiations of
csrc/traj_kernel.hip) against tests/solve_model.py.

What must be bit for bit: status, n_segs, dts (given or allocated), taus, total_time, the yaw solve, every coefficient of
a smoothing order 0 solve, and every sample / effort / traversal given the coefficients the device itself returned.
What is held to a bound: the coefficients for smoothing order >= 1.  Per problem, with exact = solve_exact (rationals),
e_dev = max |device - exact|, e_ref = max |solve_dense - exact| and scale = the largest exact coefficient,

    e_dev <= 8 * max(e_ref, 2^-52 * scale)

-- the bound is the reference's own rounding error, no problem is left out, and the factor is not tuned to the device:
a block elimination in another order stayed within 2.6 x of the dense model's error on the CPU, times three.  The
worst ratio e_dev / max(e_ref, 2^-52 scale) seen per (D, so) is printed (pytest -s) and recorded in DESIGN.md 4.15.

Shapes: K = 67 problems (a wave and three lanes), w_max = 7, W_k = k mod 8: 0 and 1 are EMPTY, 7 is w_max."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import solve_model as SM
import traj_model as TM

pytestmark = pytest.mark.gpu

K, WMAX = 67, 7
EPS = 2.0 ** -52
FACTOR = 8.0
SENTINEL = -7.25e77
MIXED = 15  # the problem with durations 0.05 and 4.9 side by side (W = 7)
MIXED_DTS = [1.1, 0.05, 4.9, 0.05, 4.9, 0.7]
CONTROLS = [0x01, 0x03, 0x07]
MAP2 = ([40, 33], [-1.5, 0.7], 0.25)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, "%s: shape %s != %s" % (what, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.shape[0] == 0, "%s: %d entries differ, first at %s: got %r want %r" % (
        what, bad.shape[0], bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def n_wp_of(k):
    return k % 8


def w_of(k):
    return min(n_wp_of(k), WMAX)


@functools.lru_cache(maxsize=None)
def problems(D):
    """Inputs, computed once and never changed: wp [4D+2][WMAX][K] state rows, n_wp [K], dts [WMAX-1][K], v_arr [K]."""
    rng = np.random.default_rng(100 + D)
    F = 4 * D + 2
    wp = np.zeros((F, WMAX, K))
    for k in range(K):
        wp[:D, :, k] = SM.random_path(rng, WMAX, D).T
    wp[D:4 * D] = np.round(rng.uniform(-1, 1, (3 * D, WMAX, K)), 2)  # vel, acc, jrk (the free ones are ignored)
    wp[4 * D] = rng.uniform(-3, 3, (WMAX, K))
    v_arr = np.round(rng.uniform(0.4, 2.5, K), 3)
    dts = np.round(rng.uniform(0.3, 2.0, (WMAX - 1, K)), 3)
    dts[:, MIXED] = MIXED_DTS
    v_arr[MIXED] = 1.0
    step = np.zeros((WMAX - 1, D))
    step[:, 0] = MIXED_DTS
    step[:, 1:] = 0.3 * np.asarray(MIXED_DTS)[:, None]
    wp[:D, 1:, MIXED] = (wp[:D, 0, MIXED][None, :] + np.cumsum(step, axis=0)).T
    n_wp = np.array([n_wp_of(k) for k in range(K)], np.int32)
    return wp, n_wp, dts, v_arr


def vals_of(wp, k, W, D):
    return np.stack([wp[a * D:(a + 1) * D, :W, k].T for a in range(3)])  # [3][W][D]


V_SCALAR = 0.8


def durations(D, mode, k, W):
    wp, _, dts, v_arr = problems(D)
    if mode == "given":
        return dts[:W - 1, k].copy()
    return SM.allocate_time(wp[:D, :W, k].T, v_arr[k] if mode == "alloc_arr" else V_SCALAR)


@functools.lru_cache(maxsize=None)
def reference(D, so, mode):
    """Per problem None (W < 2) or dict(W, dts, taus, dense, exact (so >= 1), yaw): computed once, shared."""
    wp, _, _, _ = problems(D)
    out = []
    for k in range(K):
        W = w_of(k)
        if W < 2:
            out.append(None)
            continue
        dts = durations(D, mode, k, W)
        vals, flags = vals_of(wp, k, W, D), SM.path_flags(W, so)
        out.append({"W": W, "dts": dts, "taus": SM.set_time(dts), "dense": SM.solve_dense(vals, flags, dts, so),
                    "exact": SM.solve_exact(vals, flags, dts, so) if so else None,
                    "yaw": SM.yaw_solve(wp[4 * D, :W, k], dts)[:, 0]})
    return out


def make_env(engine, D, control=0x07, v_max=2.0):
    env = engine.EnvMap(D)
    env.set_control(control)
    env.set_v_max(v_max)
    return env


def solve_set(env, D, so, mode):
    wp, n_wp, dts, v_arr = problems(D)
    return env.solve_traj(wp, n_wp=n_wp, dts=dts if mode == "given" else None,
                          v=v_arr if mode == "alloc_arr" else V_SCALAR, control=CONTROLS[so])


def coeff_of(poly, k, S):
    c = poly.coefficients()
    return c[:S, :, :, k].reshape(S * c.shape[1], c.shape[2])


def check_against_bound(got, ref_dense, exact, what):
    """The ratio e_dev / max(e_ref, 2^-52 scale); asserts it is <= FACTOR."""
    scale = SM.scale_of(exact)
    e_ref, e_dev = SM.max_err(ref_dense, exact), SM.max_err(got, exact)
    floor = max(e_ref, EPS * scale)
    assert e_dev <= FACTOR * floor, "%s: e_dev %.3g, e_ref %.3g, scale %.3g: ratio %.2f > %g" % (
        what, e_dev, e_ref, scale, e_dev / floor, FACTOR)
    return e_dev / floor


MODES = [(D, so, mode) for D in (2, 3) for so in (0, 1, 2) for mode in ("given", "alloc_arr")] + \
        [(2, so, "alloc_scalar") for so in (0, 1, 2)]


@pytest.mark.parametrize("D,so,mode", MODES, ids=["%dD-so%d-%s" % m for m in MODES])
def test_coefficients(engine, D, so, mode):
    env = make_env(engine, D)
    poly = solve_set(env, D, so, mode)
    ref = reference(D, so, mode)
    N = 2 * (so + 1)
    status, n_segs, T = poly.status, poly.n_segs, poly.total_time
    dts, taus, yaw, coef = poly.dts(), poly.taus(), poly.yaw_coefficients(), poly.coefficients()
    assert coef.shape == (WMAX - 1, N, D, K)
    worst = 0.0
    for k in range(K):
        r = ref[k]
        if r is None:  # W < 2: the status only
            assert status[k] == engine.SOLVE_EMPTY and n_segs[k] == 0 and T[k] == 0.0, k
            assert not coef[..., k].any() and not dts[:, k].any() and not taus[:, k].any() and not yaw[..., k].any(), k
            continue
        S = r["W"] - 1
        assert status[k] == 0 and n_segs[k] == S, (k, status[k], n_segs[k])
        same_bits(dts[:S, k], r["dts"], "dts of problem %d" % k)
        same_bits(taus[:S + 1, k], r["taus"], "taus of problem %d" % k)
        same_bits(T[k:k + 1], r["taus"][-1:], "total_time of problem %d" % k)
        same_bits(yaw[:S, :, k].reshape(-1), r["yaw"], "yaw coefficients of problem %d" % k)
        assert not coef[S:, ..., k].any() and not dts[S:, k].any(), k  # past S_k: untouched
        got = coeff_of(poly, k, S)
        if so == 0:
            same_bits(got, r["dense"], "coefficients of problem %d" % k)
        else:
            worst = max(worst, check_against_bound(got, r["dense"], r["exact"], "problem %d (W = %d)" % (k, r["W"])))
    print("worst e_dev / max(e_ref, eps scale) for D = %d, so = %d, %s: %.3f" % (D, so, mode, worst))
    poly.free()
    env.close()


def test_waypoint_flags(engine):
    """setWaypoints mode, K = 5, W = 5, so = 2, D = 3: interior waypoints with (pos), (pos, vel), (vel only), an end with
    a free acceleration -- the same bound --, and a problem without any fixed position: SINGULAR, outputs untouched (its
    durations are powers of two and only positions are free, so the last pivot is an exact zero, not a rounding residue)."""
    m, D, so, W, Kf = engine, 3, 2, 5, 5
    P, V, A = m.USE_POS, m.USE_VEL, m.USE_ACC
    flags = np.array([[7, P, P, P, 7], [7, P | V, P | V, P | V, 7], [7, P, V, P, 7], [7, P, P | V, P, P | V],
                      [V | A, V | A, V | A, V | A, V | A]], np.uint8).T.copy()  # [W][K]
    rng = np.random.default_rng(9)
    wp = np.zeros((14, W, Kf))
    for k in range(Kf):
        wp[:D, :, k] = SM.random_path(rng, W, D).T
    wp[D:3 * D] = np.round(rng.uniform(-1, 1, (2 * D, W, Kf)), 2)
    dts = np.round(rng.uniform(0.4, 1.8, (W - 1, Kf)), 3)
    dts[:, 4] = [1.0, 2.0, 0.5, 1.0]
    env = make_env(m, D)
    poly = env.solve_traj(wp, dts=dts, control=m.JRK, wp_flags=flags)
    assert poly.status.tolist() == [0, 0, 0, 0, m.SOLVE_SINGULAR]
    assert poly.n_segs.tolist() == [4, 4, 4, 4, 0] and not poly.coefficients()[..., 4].any() and not poly.dts()[:, 4].any()
    for k in range(4):
        vals = vals_of(wp, k, W, D)
        exact = SM.solve_exact(vals, flags[:, k], dts[:, k], so)
        dense = SM.solve_dense(vals, flags[:, k], dts[:, k], so)
        ratio = check_against_bound(coeff_of(poly, k, W - 1), dense, exact, "flags problem %d" % k)
        print("flags problem %d: ratio %.3f" % (k, ratio))
    assert SM.solve_exact(vals_of(wp, 4, W, D), flags[:, 4], dts[:, 4], so) is None  # singular in exact arithmetic too
    s = poly.sample(N=4, out=np.full((15, Kf, 5), SENTINEL))  # a failed problem has no samples
    assert (s["samples"][:, 4, :] == SENTINEL).all() and not (s["samples"][:2 * D, :4, :] == SENTINEL).any()
    poly.free()
    env.close()


def _raw_solve(m, env, poly, device, wp, n_wp, dts, v_arr, control, stride, w_max, so, D):
    """mplx_solve / mplx_solve_device with every stride = `stride` > K and sentinel-filled outputs; returns the outputs."""
    A, L = m._abi, m._abi.lib()
    Kp, N = wp.shape[2], 2 * (so + 1)
    shapes = {"status": ((stride,), np.uint8), "n_segs": ((stride,), np.int32), "total_time": ((stride,), np.float64),
              "coeff": (((w_max - 1) * N * D, stride), np.float64), "dts_out": ((w_max - 1, stride), np.float64),
              "yaw_coeff": ((2 * (w_max - 1), stride), np.float64), "taus": ((w_max, stride), np.float64)}
    host = {}
    for key, (shape, dt) in shapes.items():
        host[key] = np.full(shape, 0x5A if dt == np.uint8 else (-77 if dt == np.int32 else SENTINEL), dt)
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, np.full(a.shape[:-1] + (stride - Kp,), 0, a.dtype)], axis=-1))
    ins = {"waypoints": pad(wp), "n_wp": pad(n_wp), "v_arr": pad(v_arr)}
    if dts is not None:
        ins["dts"] = pad(dts)
    i, o = A.SolveIn(), A.SolveOut()
    i.n_prob, i.w_max, i.wp_stride, i.dt_stride, i.control, i.yaw_control = Kp, w_max, stride, stride, control, 0x01
    o.coeff_stride = o.dts_out_stride = o.yaw_stride = o.taus_stride = stride
    bufs = []
    if device:
        for key, a in list(ins.items()) + list(host.items()):
            b = m.DeviceArray(env, a.nbytes)
            b.upload(a)
            bufs.append((key, b))
            setattr(i if key in ins else o, key, b.ptr)
        A.check(env._ctx, L.mplx_solve_device(poly._h, C.byref(i), C.byref(o)))
        env.synchronize()
        for key, b in bufs:
            if key in host:
                host[key] = b.download(host[key].dtype, host[key].shape)
            b.free()
    else:
        for key, a in ins.items():
            setattr(i, key, a.ctypes.data)
        for key, a in host.items():
            setattr(o, key, a.ctypes.data)
        A.check(env._ctx, L.mplx_solve(poly._h, C.byref(i), C.byref(o)))
    return host


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_statuses_and_untouched_memory(engine, device):
    """BAD_TIME from a repeated waypoint under allocation, from v_arr[k] = 0 and from a negative given dt; EMPTY; strides
    larger than K: entries past K, every output of a failed problem and rows past S_k keep the sentinel."""
    m, D, so, w_max, Kp, stride = engine, 2, 1, 4, 6, 9
    rng = np.random.default_rng(4)
    wp = np.zeros((10, w_max, Kp))
    for k in range(Kp):
        wp[:D, :, k] = SM.random_path(rng, w_max, D).T
    wp[D:2 * D] = np.round(rng.uniform(-1, 1, (D, w_max, Kp)), 2)
    wp[:D, 2, 1] = wp[:D, 1, 1]  # problem 1: waypoint 2 repeats waypoint 1
    n_wp = np.array([4, 4, 4, 4, 1, 3], np.int32)
    v_arr = np.array([1.0, 1.0, 0.0, 0.7, 1.0, 1.3])
    dts = np.round(rng.uniform(0.5, 1.5, (w_max - 1, Kp)), 2)
    dts[1, 0] = -0.4
    env = make_env(m, D)
    poly = env.alloc_poly(Kp, w_max)
    BT, EM = m.SOLVE_BAD_TIME, m.SOLVE_EMPTY
    for given, want in ((False, [0, BT, BT, 0, EM, 0]), (True, [BT, 0, 0, 0, EM, 0])):
        h = _raw_solve(m, env, poly, device, wp, n_wp, dts if given else None, v_arr, m.ACC, stride, w_max, so, D)
        assert h["status"][:Kp].tolist() == want and (h["status"][Kp:] == 0x5A).all()
        for k in range(stride):
            S = 0 if (k >= Kp or want[k]) else int(n_wp[k]) - 1
            assert h["n_segs"][k] == (S if S else -77), k
            assert (h["total_time"][k] == SENTINEL) == (S == 0), k
            for key, rows in (("coeff", S * 4 * D), ("dts_out", S), ("yaw_coeff", 2 * S), ("taus", S + 1 if S else 0)):
                col = h[key][:, k]
                assert not (col[:rows] == SENTINEL).any() and (col[rows:] == SENTINEL).all(), (given, k, key)
            if S:
                d = dts[:S, k] if given else SM.allocate_time(wp[:D, :S + 1, k].T, v_arr[k])
                same_bits(h["dts_out"][:S, k], d, "dts of problem %d" % k)
                ref = SM.solve_dense(vals_of(wp, k, S + 1, D), SM.path_flags(S + 1, so), d, so)
                exact = SM.solve_exact(vals_of(wp, k, S + 1, D), SM.path_flags(S + 1, so), d, so)
                check_against_bound(h["coeff"][:S * 4 * D, k].reshape(S * 4, D), ref, exact, "problem %d" % k)
    poly.free()
    env.close()


def model_set(poly, D, so):
    """The model's trajectories (SM.PolySet) built from what the device returned: coefficients, yaw, dts."""
    dts, yaw, n_segs = poly.dts(), poly.yaw_coefficients(), poly.n_segs
    out = []
    for k in range(poly.n):
        S = int(n_segs[k])
        out.append(SM.PolySet(coeff_of(poly, k, S), yaw[:S, :, k].reshape(-1), dts[:S, k], so, D) if S else None)
    return out


def query_times(tr, rng):
    """Q = 9 times of one trajectory: negative, 0, two exact segment boundaries, T, past T, NaN, two inside."""
    taus = tr.taus
    return [-0.37, 0.0, float(taus[1]), float(taus[len(taus) // 2]), tr.T, tr.T + 0.25, np.nan] + [float(x) for x in rng.uniform(0, tr.T, 2)]


@pytest.mark.parametrize("D,so", [(D, so) for D in (2, 3) for so in (0, 1, 2)], ids=lambda x: str(x))
def test_evaluation_is_exact_given_the_coefficients(engine, D, so):
    m = engine
    env = make_env(m, D)
    poly = solve_set(env, D, so, "given")
    trajs = model_set(poly, D, so)
    rows = 4 * D + 3
    rng = np.random.default_rng(3)
    times = np.zeros((K, 9))
    for k, tr in enumerate(trajs):
        if tr is not None:
            times[k] = query_times(tr, rng)
    for form, n_rows in ((m.TRAJ_COMMAND, rows), (m.TRAJ_WAYPOINT, rows - 2)):
        for N, tq in ((70, None), (None, times)):
            count = 71 if N else 9
            got = poly.sample(N=N, times=tq, form=form, out=np.full((rows, K, count), SENTINEL))
            want = np.full((rows, K, count), SENTINEL)
            for k, tr in enumerate(trajs):
                if tr is not None:
                    want[:n_rows, k, :] = tr.sample(N, form) if N else tr.evaluate(times[k], form)
            same_bits(got["samples"], want, "samples (form %d, N %r)" % (form, N))
            assert np.array_equal(got["status"], poly.status)
    info = poly.info(want_states=True)
    wp, n_wp, _, _ = problems(D)
    ref = reference(D, so, "given")
    assert np.array_equal(info["status"], poly.status) and np.array_equal(info["n_segs"], poly.n_segs)
    for k, tr in enumerate(trajs):
        if tr is None:
            assert not info["effort"][:, k].any() and not info["seg_state"][:, :, k].any()
            continue
        same_bits(info["effort"][:, k], tr.effort, "efforts of problem %d" % k)
        same_bits(info["seg_state"][:, :tr.S + 1, k], wp[:, :tr.S + 1, k], "waypoints of problem %d" % k)
        assert info["total_time"][k] == tr.T
        if so == 0:
            continue
        # J of the minimised order against the exact optimum.  The efforts are the model's arithmetic bit for bit, and at
        # the optimum J moves with the square of a coefficient error, so what is left is the rounding of primitive.h's
        # formula: the same bound, on the magnitude the formula adds up (the effort of the absolute coefficients)
        vals, flags = vals_of(wp, k, tr.S + 1, D), SM.path_flags(tr.S + 1, so)
        _, cost = SM.solve_exact(vals, flags, ref[k]["dts"], so, want_cost=True)
        dense = SM.PolySet(ref[k]["dense"], ref[k]["yaw"], ref[k]["dts"], so, D)
        mag = sum(TM.effort_1d(np.abs(c[i]), np.float64(t), so + 1) for c, t in zip(tr.coef, tr.dts) for i in range(D))
        e_ref, e_dev = abs(float(dense.effort[so]) - float(cost)), abs(float(info["effort"][so, k]) - float(cost))
        assert e_dev <= FACTOR * max(e_ref, EPS * float(mag)), (k, e_dev, e_ref, float(mag))
    poly.free()
    env.close()


@functools.lru_cache(maxsize=None)
def traverse_world():
    """A 2-D map with one occupied block, a potential map, and K = 67 paths of 2 .. 7 waypoints across it: problem 0
    starts inside the block, problem 1 ends inside it, problem 2 leaves the map."""
    md, org, res = MAP2
    rng = np.random.default_rng(21)
    grid = np.zeros(md[0] * md[1], np.int8).reshape(md[1], md[0])
    grid[12:18, 14:22] = 100  # x in [2.0, 4.0), y in [3.7, 5.2)
    pot = np.zeros_like(grid)
    band = rng.random(grid.shape) < 0.5
    pot[band] = rng.integers(1, 100, grid.shape)[band]
    pot[grid == 100] = 100
    wp = np.zeros((10, WMAX, K))
    n_wp = np.array([2 + k % 6 for k in range(K)], np.int32)
    for k in range(K):
        p = SM.random_path(rng, WMAX, 2, step=(0.2, 0.6))
        wp[:2, :, k] = (p - p[0] + [rng.uniform(-0.5, 7.5), rng.uniform(1.5, 8.0)]).T
    wp[:2, :, 0] = np.array([[3.0 + 0.9 * w, 4.4 + 0.3 * w] for w in range(WMAX)]).T      # first sample in the block
    n_wp[1], n_wp[2] = 4, 7
    wp[:2, :4, 1] = np.array([[0.2, 1.4], [1.0, 2.6], [1.6, 3.4], [2.6, 4.3]]).T          # last sample in the block
    wp[:2, :, 2] = np.array([[6.5 + 0.6 * w, 2.0 + 0.2 * w] for w in range(WMAX)]).T      # leaves the map at x = 8.5
    wp[2:6] = np.round(rng.uniform(-0.5, 0.5, (4, WMAX, K)), 2)
    return grid.ravel().copy(), pot.ravel().copy(), wp, n_wp


@pytest.mark.parametrize("potential", [False, True], ids=["occupancy", "potential"])
def test_traversal(engine, potential):
    m = engine
    md, org, res = MAP2
    grid, pot, wp, n_wp = traverse_world()
    env = make_env(m, 2, control=m.JRK)
    env.setMap(org, md, grid, res)
    env.set_potential_weight(0.1)
    env.set_gradient_weight(0.25)
    if potential:
        env.set_potential_map(pot)
    poly = env.solve_traj(wp, n_wp=n_wp, v=0.9, control=m.JRK)
    assert not poly.status.any()
    trajs = model_set(poly, 2, 2)
    spans = []
    for v_max in (0.05, 2.0, 60.0):
        env.set_v_max(v_max)
        want = TM.traverse_set(trajs, grid, pot if potential else None, md, org, res, v_max, 0.1, 0.25)
        spans += [int(want["n_samples"].min()), int(want["n_samples"].max())]
        for lanes in (0, 4, 16, 64):
            got = poly.traverse(lanes=lanes)
            for key in ("status", "n_samples", "n_cells", "stop_sample"):
                assert np.array_equal(got[key], want[key]), (v_max, lanes, key)
            same_bits(got["cost"], want["cost"], "cost (v_max %g, lanes %d)" % (v_max, lanes))
        assert want["stop_sample"][0] == 0 and want["cost"][0] == np.inf           # collision at the first sample
        assert want["cost"][2] == np.inf and want["stop_sample"][2] > 0              # leaves the map
        if v_max == 0.05:  # two samples, the ends: collision at the last one
            assert want["n_samples"][1] == 2 and want["stop_sample"][1] == 1 and want["cost"][1] == np.inf
        assert np.isfinite(want["cost"]).sum() > 5
    assert min(spans) == 2 and max(spans) > 300, spans
    poly.free()
    env.close()


def test_pipeline_search_then_smooth(engine):
    """search_many on the corridor with 4 queries, smooth(v = [0.5, 1, 2]): 12 problems on the chain states."""
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    m = engine
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    starts = np.concatenate([starts, starts[:, 1:2]], axis=1)  # a fourth query: the shifted start to the original goal
    goals = np.concatenate([goals, goals[0:1]])
    kw = dict(eps=1.0, delta=10.0, capacity=1 << 16)
    multi = env.search_many(starts, goals, **kw)
    assert multi.found == [True] * 4
    vs = [0.5, 1.0, 2.0]
    poly = multi.smooth(v=vs)
    assert poly.n == 12 and not poly.status.any()
    info = poly.info(want_states=True)
    trav = poly.traverse()
    assert (trav["n_samples"] > 1).all() and not trav["status"].any()
    so, D = 1, 2
    for q in range(4):
        s0, act = multi.path(q)
        chain = env.traj_info(s0, act.reshape(-1, 1), want_states=True)["seg_state"][:, :, 0]  # [F][S + 1]
        W = len(act) + 1
        for vi, v in enumerate(vs):
            k = vi * 4 + q
            assert poly.n_segs[k] == W - 1
            same_bits(info["seg_state"][:, :W, k], chain, "waypoints of problem %d" % k)
            vals = np.stack([chain[a * D:(a + 1) * D, :].T for a in range(3)])
            dts = SM.allocate_time(chain[:D].T, v)
            same_bits(poly.dts()[:W - 1, k], dts, "dts of problem %d" % k)
            flags = SM.path_flags(W, so)
            exact, dense = SM.solve_exact(vals, flags, dts, so), SM.solve_dense(vals, flags, dts, so)
            check_against_bound(coeff_of(poly, k, W - 1), dense, exact, "problem %d" % k)
            # at a tau the trajectory is at its waypoint: the polynomial of the segment that ends there, whose value
            # moves by at most sum_n |dp_n| T^n with the coefficient errors dp_n <= the bound above
            taus = poly.taus()[:W, k]
            s = poly.sample(times=np.tile(taus, (12, 1)), form=m.TRAJ_COMMAND)["samples"][:D, k, :]
            scale = SM.scale_of(exact)
            tol = FACTOR * max(SM.max_err(dense, exact), EPS * scale) * sum(max(float(dts.max()), 1.0) ** n for n in range(4))
            # ... plus the rounding of tau_w - tau_{w-1} (a few ulps of T, times a velocity below `scale`) and of the value
            tol += 8 * EPS * (float(taus[-1]) * scale + np.abs(chain[:D]).max())
            assert np.abs(s - chain[:D]).max() <= tol, (k, np.abs(s - chain[:D]).max(), tol)
    again = env.search_many(starts, goals, **kw)  # the context is as it was
    assert again.cost == multi.cost and again.expanded == multi.expanded and again.rounds == multi.rounds
    for q in range(4):
        assert np.array_equal(again.path(q)[1], multi.path(q)[1])
    again.free()
    poly.free()
    multi.free()
    env.close()


def test_action_chain_paths_are_unchanged(engine):
    """traj_sample / traj_traverse of an action-chain set before and after a solve on the same context: bit for bit."""
    m = engine
    U, starts, actions, (md, org, res), grid, pot = TM.gpu_case(0x03, 2)
    env = make_env(m, 2, control=0x03)
    env.setMap(org, md, grid, res)
    env.set_dt(0.7)
    env.set_u(U)
    env.set_potential_map(pot)

    def chain_results():
        return (env.traj_sample(starts, actions, N=33), env.traj_sample(starts, actions, times=[0.0, 0.7, 1.9], form=m.TRAJ_WAYPOINT),
                env.traj_traverse(starts, actions, lanes=16), env.traj_info(starts, actions))

    before = chain_results()
    poly = solve_set(env, 2, 1, "given")
    poly.sample(N=5)
    poly.traverse()
    after = chain_results()
    for b, a in zip(before, after):
        for key in b:
            assert np.array_equal(np.asarray(b[key]).view(np.uint8), np.asarray(a[key]).view(np.uint8)), key
    poly.free()
    env.close()


def test_traj_solver_class(engine):
    """planner.TrajSolver on the reference's own test path (test/test_traj_solver.cpp): setPath zeroes the derivatives."""
    m = engine
    ts = m.TrajSolver(2, m.JRK)
    ts.setPath(SM.REF_PATH)
    ts.setV(1.0)
    poly = ts.solve()
    assert poly.status.tolist() == [0] and ts.getDts() == [1.0, 1.0, 3.0] and len(ts.getWaypoints()) == 4
    vals, flags = SM.path_vals(SM.REF_PATH), SM.path_flags(4, 2)
    dts = SM.allocate_time(SM.REF_PATH, 1.0)
    check_against_bound(coeff_of(poly, 0, 3), SM.solve_dense(vals, flags, dts, 2), SM.solve_exact(vals, flags, dts, 2), "ref path")
    ts.setDts([0.5, 2.0, 1.0])
    p2 = ts.solve()
    same_bits(p2.dts()[:, 0], [0.5, 2.0, 1.0], "given dts")
    p2.free()
    poly.free()
    ts.close()


def test_argument_errors(engine):
    m = engine
    A, L = m._abi, m._abi.lib()
    env = make_env(m, 2)
    poly = env.alloc_poly(4, 3)
    wp = np.zeros((10, 3, 4))
    wp[0] = np.arange(3)[:, None] + 1.0

    def call(fn=None, **kw):
        i, o = A.SolveIn(), A.SolveOut()
        i.waypoints, i.n_prob, i.w_max, i.wp_stride, i.v, i.control, i.yaw_control = wp.ctypes.data, 4, 3, 4, 1.0, 0x03, 0x01
        for key, val in kw.items():
            setattr(i, key, val)
        return (fn or L.mplx_solve)(poly._h, C.byref(i), C.byref(o))

    assert call() == A.OK
    assert call(control=0x0F) == A.ERR_ARG and call(control=0x1F) == A.ERR_ARG and call(control=0x05) == A.ERR_ARG  # SNP is not built
    assert call(yaw_control=0x03) == A.ERR_ARG and b"yaw_control" in L.mplx_last_error(env._ctx)
    assert call(w_max=1) == A.ERR_ARG and call(w_max=4) == A.ERR_ARG
    assert call(n_prob=5, wp_stride=5) == A.ERR_ARG  # above k_cap
    assert call(waypoints=None) == A.ERR_ARG and call(wp_stride=3) == A.ERR_ARG
    assert call(fn=L.mplx_solve_device, control=0x0F) == A.ERR_ARG
    assert L.mplx_solve(poly._h, None, None) == A.ERR_ARG
    assert call(n_prob=0) == A.OK
    h = C.c_void_p()
    assert L.mplx_poly_create(env._ctx, 0, 3, C.byref(h)) == A.ERR_ARG and L.mplx_poly_create(env._ctx, 4, 1, C.byref(h)) == A.ERR_ARG
    with pytest.raises(ValueError):
        env.solve_traj(wp, control=m.SNP)
    with pytest.raises(A.MplxError) as e:  # traverse without a map
        poly.n, poly.n_wmax = 4, 3
        poly.traverse()
    assert e.value.code == A.ERR_STATE
    fresh = env.alloc_poly(2, 2)
    t = A.TrajTraverseOut()
    assert L.mplx_poly_traverse(fresh._h, 0, C.byref(t)) == A.ERR_STATE  # nothing solved
    fresh.free()
    poly.free()
    env.close()
