"""Trajectory sets at long chains and many waves: the solver (csrc/solve_kernel.hip), the POLY instantiations of
csrc/traj_kernel.hip, loads and limits (csrc/limits_kernel.hip) and time scaling (csrc/scale_kernel.hip) on one set of

    K = 200 problems (three full waves and eight lanes), w_max = 33, n_wp[k] cycling through
    [0, 1, 2, 3, 8, 9, 16, 17, 24, 32, 33, 40]  (0, 1: EMPTY; 40: clamped to w_max; S = 31 next to S = 32),

in a poly allocated larger than the call (alloc_poly(256, 40)), so every table stride is the call's n = 200 and not the
capacity.  Their own test files run at K <= 70 and at most 6 segments (tests/test_gpu_solve.py, test_gpu_limits.py,
test_gpu_scale.py); nothing there carries the recursion past six waypoints, bisects more than three steps, reduces over
a late segment or fills Ts[0 .. 32].

The inputs are solve_model.long_problems(D): derivative rows as test_gpu_solve.problems; durations random in [0.3, 2.0]
rounded to 1e-3, and per W class one problem alternating 0.05 s / 4.9 s and one growing geometrically from 0.05 s to 5 s.

What is held bit for bit: everything tests/test_gpu_solve.py holds bit for bit, and now the coefficients of smoothing
order >= 1 as well, against solve_model.solve_block, the float64 restatement of the kernel's own operation order (the
kernel is plain IEEE: -ffp-contract=off, true divisions).  solve_block is a twin, not a reference, so a fixed subset
(solve_model.LONG_EXACT: W <= 24, every duration pattern, 6 problems with given durations and 2 with allocated ones per
(D, so)) also goes against solve_exact under the project's bound e_dev <= 8 * max(e_ref, 2^-52 * scale) with e_ref the
error of solve_dense.  The seed (solve_model.LONG_SEED = 300, + D) was fixed on the CPU with solve_block before any
device run; the twin's worst ratios e / max(e_ref, 2^-52 scale) on that subset were

    D = 2: so = 1 given 1.158, allocated 2.886; so = 2 given 5.973, allocated 3.694
    D = 3: so = 1 given 3.489, allocated 2.869; so = 2 given 2.309, allocated 2.788

(the 5.973 is W = 8 alternating, where solve_dense itself is 788 * 2^-52 * scale from the exact solution), and the flags
set below is at 0.497, 0.228, 0.552 and 1.113.  A host build of solve_kernel.hip (-ffp-contract=off) equals solve_block
bit for bit on all 200 problems of every (D, so, duration mode) and on the flags set.  On an MI355X the device is the
twin bit for bit, so its ratios are these, digit for digit (printed with pytest -s)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import limits_model as LM
import scale_model as SCM
import solve_model as SM
import traj_model as TM
from test_gpu_solve import CONTROLS, SENTINEL, _raw_solve, check_against_bound, coeff_of, make_env, model_set, same_bits
from test_gpu_solve import problems as old_problems
from test_gpu_limits import _raw_load
from test_gpu_scale import FILL, FILL_F64, FILL_I32, same_rows

pytestmark = pytest.mark.gpu

K, WMAX = SM.LONG_K, SM.LONG_WMAX
K_CAP, W_CAP = 256, 40
F64 = np.float64
REF, ALL = LM.REFERENCE, LM.ALL_ROOTS
KEYS = ("max_vel", "max_acc", "max_jrk")
JRKxYAW = 0x17
W_OF = [SM.long_w(k) for k in range(K)]
S_OF = [max(w - 1, 0) for w in W_OF]
LIVE = [k for k in range(K) if S_OF[k] > 0]


def test_the_shapes_are_the_ones_this_file_is_about():
    assert K == 200 and WMAX == 33 and sorted(set(W_OF)) == [0, 1, 2, 3, 8, 9, 16, 17, 24, 32, 33]
    assert {31, 32, 23} <= set(S_OF) and W_OF[11] == 33 and SM.long_problems(2)[1][11] == 40
    for mode, ks in SM.LONG_EXACT.items():
        assert len(ks) <= 8 and all(2 <= W_OF[k] <= 24 for k in ks)
        assert {SM.long_pattern(k) for k in ks} >= {"alternating", "geometric"}
    assert {SM.long_pattern(k) for k in SM.LONG_EXACT["given"]} == {"random", "alternating", "geometric"}
    assert sum(len(ks) for ks in SM.LONG_EXACT.values()) <= 8


# ------------------------------------------------------------------------------------------------ calls into a given poly
def solve_into(m, env, poly, wp, n_wp, dts, v, control, wp_flags=None):
    """EnvMap.solve_traj (mplx_solve, host pointers) into a poly the caller allocated, with its bookkeeping."""
    A = m._abi
    so = SM.so_of(control)
    wp = np.ascontiguousarray(wp, dtype=np.float64)
    W, Kp = wp.shape[1], wp.shape[2]
    i, o = A.SolveIn(), A.SolveOut()
    i.waypoints, i.n_prob, i.w_max, i.wp_stride = wp.ctypes.data, Kp, W, Kp
    keep = [wp]
    if n_wp is not None:
        keep.append(np.ascontiguousarray(n_wp, dtype=np.int32))
        i.n_wp = keep[-1].ctypes.data
    if dts is not None:
        keep.append(np.ascontiguousarray(dts, dtype=np.float64).reshape(W - 1, Kp))
        i.dts, i.dt_stride = keep[-1].ctypes.data, Kp
    if np.ndim(v) == 0:
        i.v = float(v)
    else:
        keep.append(np.ascontiguousarray(v, dtype=np.float64))
        i.v_arr = keep[-1].ctypes.data
    if wp_flags is not None:
        keep.append(np.ascontiguousarray(wp_flags, dtype=np.uint8).reshape(W, Kp))
        i.wp_flags, i.flag_stride = keep[-1].ctypes.data, Kp
    i.control, i.yaw_control = int(control), 0x01
    N, S = 2 * (so + 1), W - 1
    host = {"status": np.zeros(Kp, np.uint8), "n_segs": np.zeros(Kp, np.int32), "total_time": np.zeros(Kp, np.float64),
            "coeff": np.zeros((S, N, env.dim, Kp)), "dts": np.zeros((S, Kp)), "yaw_coeff": np.zeros((S, 2, Kp)),
            "taus": np.zeros((W, Kp))}
    o.status, o.n_segs, o.total_time = host["status"].ctypes.data, host["n_segs"].ctypes.data, host["total_time"].ctypes.data
    o.coeff, o.dts_out, o.yaw_coeff, o.taus = (host[key].ctypes.data for key in ("coeff", "dts", "yaw_coeff", "taus"))
    o.coeff_stride = o.dts_out_stride = o.yaw_stride = o.taus_stride = Kp
    A.check(env._ctx, A.lib().mplx_solve(poly._h, C.byref(i), C.byref(o)))
    poly.n, poly.so, poly.n_wmax, poly._host, poly.control, poly._lambda = Kp, so, W, host, int(control), None
    return poly


def load_into(m, env, poly, coeff, dts, n_segs, control):
    """EnvMap.load_traj (mplx_poly_load, host pointers) into a poly the caller allocated, with its bookkeeping."""
    A = m._abi
    c = np.ascontiguousarray(coeff, dtype=np.float64)
    S, Kp = c.shape[0], c.shape[3]
    dts = np.ascontiguousarray(dts, dtype=np.float64).reshape(S, Kp)
    n_segs = np.ascontiguousarray(n_segs, dtype=np.int32)
    i, o = A.PolyLoadIn(), A.PolyLoadOut()
    i.n_prob, i.w_max, i.control, i.n_segs = Kp, S + 1, int(control), n_segs.ctypes.data
    i.dts, i.dt_stride, i.coeff, i.coeff_stride = dts.ctypes.data, Kp, c.ctypes.data, Kp
    host = {"status": np.zeros(Kp, np.uint8), "n_segs": np.zeros(Kp, np.int32), "total_time": np.zeros(Kp, np.float64),
            "taus": np.zeros((S + 1, Kp))}
    o.status, o.n_segs, o.total_time = host["status"].ctypes.data, host["n_segs"].ctypes.data, host["total_time"].ctypes.data
    o.taus, o.taus_stride = host["taus"].ctypes.data, Kp
    A.check(env._ctx, A.lib().mplx_poly_load(poly._h, C.byref(i), C.byref(o)))
    seg = np.arange(S)[:, None] < host["n_segs"][None, :]
    host["dts"] = np.where(seg, dts, 0.0)
    host["segments"] = np.where(seg[:, None, None, :], c, 0.0)
    poly.n, poly.so, poly.n_wmax, poly._host, poly.control, poly._lambda = Kp, None, S + 1, host, int(control), None
    return poly


def solve_long(m, env, D, so, mode, poly=None):
    wp, n_wp, dts, v_arr = SM.long_problems(D)
    poly = env.alloc_poly(K_CAP, W_CAP) if poly is None else poly
    return solve_into(m, env, poly, wp, n_wp, dts if mode == "given" else None, v_arr, CONTROLS[so])


# ------------------------------------------------------------------------------------------------------------ models
@functools.lru_cache(maxsize=None)
def model(D, so, mode):
    """Per problem None (W < 2) or dict(W, dts, taus, coef, yaw): coef is solve_dense for so = 0 and solve_block for
    so >= 1.  Computed once per (D, so, mode) and shared."""
    wp = SM.long_problems(D)[0]
    out = []
    for k in range(K):
        W = W_OF[k]
        if W < 2:
            out.append(None)
            continue
        dts = SM.long_durations(D, mode, k)
        vals, flags = SM.long_vals(wp, k, W, D), SM.path_flags(W, so)
        coef = SM.solve_dense(vals, flags, dts, so) if so == 0 else SM.solve_block(vals, flags, dts, so)
        out.append({"W": W, "dts": dts, "taus": SM.set_time(dts), "coef": coef, "yaw": SM.yaw_solve(wp[4 * D, :W, k], dts)[:, 0]})
    return out


@functools.lru_cache(maxsize=None)
def exact_of(D, so, mode, k):
    """(solve_dense, solve_exact) of problem k of the exact subset."""
    wp = SM.long_problems(D)[0]
    W = W_OF[k]
    vals, flags, dts = SM.long_vals(wp, k, W, D), SM.path_flags(W, so), SM.long_durations(D, mode, k)
    return SM.solve_dense(vals, flags, dts, so), SM.solve_exact(vals, flags, dts, so)


# ------------------------------------------------------------------------------------------------------ coefficients
MODES = [(D, so, mode) for D in (2, 3) for so in (0, 1, 2) for mode in ("given", "alloc_arr")]


@pytest.mark.parametrize("D,so,mode", MODES, ids=["%dD-so%d-%s" % x for x in MODES])
def test_coefficients(engine, D, so, mode):
    m = engine
    env = make_env(m, D)
    poly = solve_long(m, env, D, so, mode)
    ref = model(D, so, mode)
    N = 2 * (so + 1)
    status, n_segs, T = poly.status, poly.n_segs, poly.total_time
    dts, taus, yaw, coef = poly.dts(), poly.taus(), poly.yaw_coefficients(), poly.coefficients()
    assert coef.shape == (WMAX - 1, N, D, K)
    for k in range(K):
        r = ref[k]
        if r is None:  # W < 2: the status only
            assert status[k] == m.SOLVE_EMPTY and n_segs[k] == 0 and T[k] == 0.0, k
            assert not coef[..., k].any() and not dts[:, k].any() and not taus[:, k].any() and not yaw[..., k].any(), k
            continue
        S = r["W"] - 1
        assert status[k] == 0 and n_segs[k] == S, (k, status[k], n_segs[k])
        same_bits(dts[:S, k], r["dts"], "dts of problem %d" % k)
        same_bits(taus[:S + 1, k], r["taus"], "taus of problem %d" % k)
        same_bits(T[k:k + 1], r["taus"][-1:], "total_time of problem %d" % k)
        same_bits(yaw[:S, :, k].reshape(-1), r["yaw"], "yaw coefficients of problem %d" % k)
        assert not coef[S:, ..., k].any() and not dts[S:, k].any() and not taus[S + 1:, k].any() and not yaw[S:, :, k].any(), k
        same_bits(coeff_of(poly, k, S), r["coef"], "coefficients of problem %d (W = %d, %s)" % (k, r["W"], SM.long_pattern(k)))
    worst = 0.0
    if so:
        for k in SM.LONG_EXACT.get(mode, []):
            dense, exact = exact_of(D, so, mode, k)
            ratio = check_against_bound(coeff_of(poly, k, S_OF[k]), dense, exact, "problem %d (W = %d, %s)" % (k, W_OF[k], SM.long_pattern(k)))
            worst = max(worst, ratio)
        print("long set: worst e_dev / max(e_ref, eps scale) for D = %d, so = %d, %s: %.3f" % (D, so, mode, worst))
    poly.free()
    env.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_raw_forms_with_strides(engine, device):
    """mplx_solve / mplx_solve_device with every stride = 211 and sentinel-filled outputs: columns >= K, rows past S_k
    and failed problems keep the sentinel, solved rows are the wrapped call's bit for bit."""
    m, D, so, stride = engine, 3, 2, 211
    wp, n_wp, dts, v_arr = SM.long_problems(D)
    env = make_env(m, D)
    wrapped = solve_long(m, env, D, so, "given")
    poly = env.alloc_poly(K_CAP, W_CAP)
    N = 2 * (so + 1)
    for given in (True, False):
        if not given:
            solve_long(m, env, D, so, "alloc_arr", poly=wrapped)
        h = _raw_solve(m, env, poly, device, np.asarray(wp), np.asarray(n_wp), np.asarray(dts) if given else None,
                       np.asarray(v_arr), m.JRK, stride, WMAX, so, D)
        assert (h["status"][K:] == 0x5A).all() and np.array_equal(h["status"][:K], wrapped.status)
        for k in range(stride):
            S = S_OF[k] if k < K else 0
            assert h["n_segs"][k] == (S if S else -77), k
            assert (h["total_time"][k] == SENTINEL) == (S == 0), k
            for key, rows in (("coeff", S * N * D), ("dts_out", S), ("yaw_coeff", 2 * S), ("taus", S + 1 if S else 0)):
                col = h[key][:, k]
                assert not (col[:rows] == SENTINEL).any() and (col[rows:] == SENTINEL).all(), (given, k, key)
            if S:
                same_bits(h["coeff"][:S * N * D, k], wrapped.coefficients()[:S, :, :, k].reshape(-1), "coefficients of problem %d" % k)
                same_bits(h["dts_out"][:S, k], wrapped.dts()[:S, k], "dts of problem %d" % k)
                same_bits(h["yaw_coeff"][:2 * S, k], wrapped.yaw_coefficients()[:S, :, k].reshape(-1), "yaw of problem %d" % k)
                same_bits(h["taus"][:S + 1, k], wrapped.taus()[:S + 1, k], "taus of problem %d" % k)
                same_bits(h["total_time"][k], wrapped.total_time[k], "total time of problem %d" % k)
    poly.free()
    wrapped.free()
    env.close()


# ------------------------------------------------------------------------------------------------------------- flags
def test_flags_at_length(engine):
    """setWaypoints mode at W = 17, so = 2, D = 3 (solve_model.long_flag_problems): solved problems bit for bit the twin
    and within the bound of solve_exact; the problem without a fixed position is SINGULAR, outputs untouched."""
    m, D, so = engine, 3, 2
    wp, flags, dts = SM.long_flag_problems()
    W, Kf = wp.shape[1], wp.shape[2]
    env = make_env(m, D)
    poly = solve_into(m, env, env.alloc_poly(K_CAP, W_CAP), wp, None, dts, 1.0, m.JRK, wp_flags=flags)
    assert poly.status.tolist() == [0, 0, 0, 0, m.SOLVE_SINGULAR]
    assert poly.n_segs.tolist() == [W - 1] * 4 + [0] and not poly.coefficients()[..., 4].any() and not poly.dts()[:, 4].any()
    assert not poly.taus()[:, 4].any() and not poly.yaw_coefficients()[..., 4].any() and poly.total_time[4] == 0.0
    for k in range(Kf - 1):
        vals = SM.long_vals(wp, k, W, D)
        twin = SM.solve_block(vals, flags[:, k], dts[:, k], so)
        same_bits(coeff_of(poly, k, W - 1), twin, "flags problem %d" % k)
        ratio = check_against_bound(coeff_of(poly, k, W - 1), SM.solve_dense(vals, flags[:, k], dts[:, k], so),
                                    SM.solve_exact(vals, flags[:, k], dts[:, k], so), "flags problem %d" % k)
        print("long flags problem %d: ratio %.3f" % (k, ratio))
    assert SM.solve_block(SM.long_vals(wp, 4, W, D), flags[:, 4], dts[:, 4], so) is None
    s = poly.sample(N=4, out=np.full((15, Kf, 5), SENTINEL))
    assert (s["samples"][:, 4, :] == SENTINEL).all() and not (s["samples"][:2 * D, :4, :] == SENTINEL).any()
    poly.free()
    env.close()


# ---------------------------------------------------------------------------------------------------------- sampling
def long_times(trajs):
    """[K][Q] per-problem times: every stored tau 0 .. S_k (the rest padded with T + 0.25), the midpoints of the first, a
    middle and the last segment, a negative time and NaN."""
    Q = WMAX + 5
    times = np.zeros((K, Q))
    for k, tr in enumerate(trajs):
        if tr is None:
            continue
        t = np.full(WMAX, tr.T + 0.25)
        t[:tr.S + 1] = tr.taus
        mids = [float(tr.taus[s] + tr.dts[s] / 2) for s in (0, tr.S // 2, tr.S - 1)]
        times[k] = list(t) + mids + [-0.37, np.nan]
    return times


@pytest.mark.parametrize("D,so", [(2, 1), (3, 2)], ids=lambda x: str(x))
def test_sampling_at_every_boundary(engine, D, so):
    m = engine
    env = make_env(m, D)
    poly = solve_long(m, env, D, so, "given")
    trajs = model_set(poly, D, so)
    assert {tr.S for tr in trajs if tr is not None} >= {31, 32, 23}  # among the queried boundaries
    times = long_times(trajs)
    rows, Q = 4 * D + 3, times.shape[1]
    differ = 0
    for form, n_rows in ((m.TRAJ_COMMAND, rows), (m.TRAJ_WAYPOINT, rows - 2)):
        for N, tq in ((130, None), (None, times)):
            count = N + 1 if N else Q
            got = poly.sample(N=N, times=tq, form=form, out=np.full((rows, K, count), SENTINEL))
            want = np.full((rows, K, count), SENTINEL)
            for k, tr in enumerate(trajs):
                if tr is not None:
                    want[:n_rows, k, :] = tr.sample(N, form) if N else tr.evaluate(times[k], form)
            same_rows(got["samples"], want, "samples (form %d, N %r)" % (form, N))
            assert np.array_equal(got["status"], poly.status)
    # the two forms pick different segments at an interior boundary, and the rows show it (a `<` for the command form's
    # `<=` would not pass): the highest derivative the solve leaves free jumps there
    for k, tr in enumerate(trajs):
        if tr is not None and tr.S >= 23:
            a, b = tr.evaluate(tr.taus[1:-1], m.TRAJ_COMMAND), tr.evaluate(tr.taus[1:-1], m.TRAJ_WAYPOINT)
            differ += int((a[:4 * D] != b[:4 * D]).any(axis=0).sum())
    assert differ > 1000
    info = poly.info(want_states=True)
    wp = SM.long_problems(D)[0]
    assert np.array_equal(info["status"], poly.status) and np.array_equal(info["n_segs"], poly.n_segs)
    for k, tr in enumerate(trajs):
        if tr is None:
            assert not info["effort"][:, k].any() and not info["seg_state"][:, :, k].any()
            continue
        same_bits(info["effort"][:, k], tr.effort, "efforts of problem %d" % k)
        same_bits(info["seg_state"][:, :tr.S + 1, k], wp[:, :tr.S + 1, k], "waypoints of problem %d" % k)
        assert not info["seg_state"][:, tr.S + 1:, k].any(), k
        assert info["total_time"][k] == tr.T
    poly.free()
    env.close()


# --------------------------------------------------------------------------------------------------------- traversal
MAP_LONG = ([160, 120], [-1.5, 0.7], 0.25)  # test_gpu_solve.MAP2's origin and resolution, 40 m x 30 m
HIT, LEAVE = 9, 10  # n_wp 32 and 33: collides in a segment >= 16; leaves the map in its last segment


@functools.lru_cache(maxsize=None)
def traverse_world_long():
    """A 2-D map with one occupied block and a potential map, and K = 200 paths of up to 33 waypoints across it (n_wp as
    everywhere in this file).  Path HIT is a line that enters the block in its segment 20, path LEAVE a line whose last
    segment crosses the map's edge."""
    md, org, res = MAP_LONG
    rng = np.random.default_rng(23)
    grid = np.zeros((md[1], md[0]), np.int8)
    grid[60:68, 100:110] = 100  # x in [23.5, 26.0), y in [15.7, 17.7)
    pot = np.zeros_like(grid)
    band = rng.random(grid.shape) < 0.5
    pot[band] = rng.integers(1, 100, grid.shape)[band]
    pot[grid == 100] = 100
    wp = np.zeros((10, WMAX, K))
    n_wp = np.array(SM.long_problems(2)[1])
    for k in range(K):
        p = SM.random_path(rng, WMAX, 2, step=(0.2, 0.6))
        wp[:2, :, k] = (p - p[0] + [rng.uniform(8.0, 28.0), rng.uniform(8.0, 22.0)]).T
    wp[:2, :, HIT] = np.array([[14.0 + 0.5 * w, 16.5 + 0.01 * w] for w in range(WMAX)]).T    # x = 23.5 at w = 19
    wp[:2, :, LEAVE] = np.array([[22.9 + 0.5 * w, 5.0 + 0.1 * w] for w in range(WMAX)]).T    # x = 38.5 between w = 31 and 32
    wp[2:6] = np.round(rng.uniform(-0.5, 0.5, (4, WMAX, K)), 2)
    return grid.ravel().copy(), pot.ravel().copy(), wp, n_wp


def test_traversal(engine):
    m = engine
    md, org, res = MAP_LONG
    grid, pot, wp, n_wp = traverse_world_long()
    env = make_env(m, 2, control=m.JRK)
    env.setMap(org, md, grid, res)
    env.set_potential_weight(0.1)
    env.set_gradient_weight(0.25)
    env.set_potential_map(pot)
    poly = solve_into(m, env, env.alloc_poly(K_CAP, W_CAP), wp, n_wp, None, 0.9, m.JRK)
    assert [int(s) for s in poly.n_segs] == S_OF
    trajs = model_set(poly, 2, 2)
    empty = TM.Traj(m.JRK, 2, 1.0, [], np.zeros(10), [])  # what a failed problem traverses as
    for v_max in (2.0, 20.0):
        env.set_v_max(v_max)
        want = TM.traverse_set([tr if tr is not None else empty for tr in trajs], grid, pot, md, org, res, v_max, 0.1, 0.25)
        for lanes in (0, 4, 16, 64):
            got = poly.traverse(lanes=lanes)
            for key in ("status", "n_samples", "n_cells", "stop_sample"):
                assert np.array_equal(got[key], want[key]), (v_max, lanes, key)
            assert np.array_equal(got["status"], poly.status), (v_max, lanes)
            same_bits(got["cost"], want["cost"], "cost (v_max %g, lanes %d)" % (v_max, lanes))
        for k, last in ((HIT, False), (LEAVE, True)):  # the model says where the two crafted paths stop
            tr = trajs[k]
            assert want["cost"][k] == np.inf and want["stop_sample"][k] > 0
            t_stop = F64(want["stop_sample"][k]) * (F64(tr.T) / F64(want["n_samples"][k] - 1))
            seg = int(np.searchsorted(tr.taus, t_stop, side="left")) - 1
            assert (seg == tr.S - 1 and tr.S == 32) if last else (16 <= seg < tr.S - 1), (k, seg, tr.S)
        assert np.isfinite(want["cost"][LIVE]).sum() > 50 and want["n_samples"].max() > (300 if v_max > 2 else 30)
    poly.free()
    env.close()


# ------------------------------------------------------------------------------------------------------------ limits
def coefs_of(poly, k):
    S = int(poly.n_segs[k])
    seg = poly.segments()
    D = seg.shape[1] - 1
    return [seg[s, :D, :, k] for s in range(S)], poly.dts()[:S, k]


def model_limits(poly, control, mv, ma, mj, mode):
    return [LM.traj_limits(*coefs_of(poly, k), control, mv, ma, mj, mode) if poly.n_segs[k] else None for k in range(poly.n)]


def check_limits(got, want, what):
    for k, w in enumerate(want):
        if w is None:
            assert not any(got[key][:, k].any() for key in KEYS) and got["valid"][k] == 0 and got["first_bad"][k] == -1, (what, k)
            continue
        for key in KEYS:
            same_bits(got[key][:, k], w[key], "%s: %s of problem %d" % (what, key, k))
        assert (got["exceed"][k], got["valid"][k], got["first_bad"][k]) == (w["exceed"], w["valid"], w["first_bad"]), (what, k)


@pytest.mark.parametrize("D,so", [(2, 0), (3, 1)], ids=lambda x: str(x))
@pytest.mark.parametrize("mode", [REF, ALL], ids=["reference", "all_roots"])
def test_limits_of_the_solved_sets_ieee_only(engine, D, so, mode):
    """Smoothing order 0 and 1: c0 = c1 = 0, the root finder stays in its linear and quadratic branches."""
    m = engine
    env = make_env(m, D)
    poly = solve_long(m, env, D, so, "given")
    free = model_limits(poly, CONTROLS[so], 0, 0, 0, mode)
    tops = np.array([[w[key].max() for key in KEYS] for w in free if w is not None])
    mv, ma, mj = (float(np.median(tops[:, q])) for q in range(3))
    check_limits(poly.limits(0.0, 0.0, 0.0, all_roots=mode == ALL), free, "free limits")
    med = model_limits(poly, CONTROLS[so], mv, ma, mj, mode)
    check_limits(poly.limits(mv, ma, mj, all_roots=mode == ALL), med, "median limits")
    if so == 1:  # an ACC set: the velocity decides, and late segments do
        bad = [w["first_bad"] for w in med if w is not None and not w["valid"]]
        assert len(bad) > 20 and max(bad) >= 16 and sum(w["valid"] for w in med if w is not None) > 20
    poly.free()
    env.close()


def s_bad(k):
    return (7 * k) % S_OF[k]


def s_bad2(k):
    """A second violating segment, later than the first, in a third of the problems (or None)."""
    return S_OF[k] - 1 if (k % 3 == 0 and S_OF[k] and s_bad(k) < S_OF[k] - 1) else None


MV_LOADED = 1.0


@functools.lru_cache(maxsize=None)
def loaded_set(D):
    """K = 200 trajectories with the n_segs of the solved set, of gentle segments with c0 = c1 = 0 (sixteenths) of which
    segment s_bad(k) -- and s_bad2(k) -- starts at 2 m/s on axis 0: coeff [32][D + 1][6][K], dts [32][K] in quarters of
    a second from 0.5 to 1.5, n_segs [K]."""
    rng = np.random.default_rng(700 + D)
    c = np.zeros((WMAX - 1, D + 1, 6, K))
    c[:, :D, 2] = rng.integers(-2, 3, (WMAX - 1, D, K)) / 16.0    # |c2| <= 0.125
    c[:, :D, 3] = rng.integers(-4, 5, (WMAX - 1, D, K)) / 16.0    # |c3| <= 0.25
    c[:, :D, 4] = rng.integers(-4, 5, (WMAX - 1, D, K)) / 16.0    # |c4| <= 0.25
    c[:, :, 5] = rng.integers(-32, 33, (WMAX - 1, D + 1, K)) / 16.0
    c[:, D, 4] = rng.integers(-8, 9, (WMAX - 1, K)) / 16.0
    dts = rng.integers(2, 7, (WMAX - 1, K)) / 4.0
    for k in LIVE:
        for s in (s_bad(k), s_bad2(k)):
            if s is not None:
                c[s, 0, 4, k] = 2.0
    # |v| <= |c2| t^2 / 2 + |c3| t + |c4| <= 0.125 * 1.125 + 0.25 * 1.5 + 0.25 < 0.77 elsewhere; >= 2 - 0.52 in a bad one
    n_segs = np.array(S_OF, np.int32)
    return c, dts, n_segs


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("mode", [REF, ALL], ids=["reference", "all_roots"])
def test_limits_of_a_loaded_set_first_bad_segment(engine, D, mode):
    m = engine
    c, dts, n_segs = loaded_set(D)
    env = make_env(m, D)
    poly = load_into(m, env, env.alloc_poly(K_CAP, W_CAP), c, dts, n_segs, m.ACC)
    assert (poly.status[n_segs == 0] == m.SOLVE_EMPTY).all() and not poly.status[n_segs > 0].any()
    assert np.array_equal(poly.n_segs, n_segs)
    want = model_limits(poly, m.ACC, MV_LOADED, 0.0, 0.0, mode)
    got = poly.limits(MV_LOADED, 0.0, 0.0, all_roots=mode == ALL)
    check_limits(got, want, "the loaded set")
    for k in LIVE:
        assert got["first_bad"][k] == s_bad(k) and got["valid"][k] == 0 and got["exceed"][k] == LM.EXCEED_VEL, k
        # exactly the planted segments are over the limit
        over = [s for s in range(S_OF[k]) if max(LM.axis_max(c[s, i, :, k], dts[s, k], 1, mode) for i in range(D)) > MV_LOADED]
        assert over == sorted({s_bad(k)} | ({s_bad2(k)} if s_bad2(k) is not None else set())), k
    firsts = {(s_bad(k), S_OF[k]) for k in LIVE}
    assert any(s == 0 and S > 8 for s, S in firsts) and any(s == S - 1 and S >= 23 for s, S in firsts)
    assert sum(s >= 16 for s, _ in firsts) >= 5 and sum(s_bad2(k) is not None for k in LIVE) > 30
    check_limits(poly.limits(0.0, 0.0, 0.0, all_roots=mode == ALL), model_limits(poly, m.ACC, 0, 0, 0, mode), "the loaded set, free")
    poly.free()
    env.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_raw_load_forms_with_strides(engine, device):
    """mplx_poly_load / mplx_poly_load_device with every stride = 211 and sentinel-filled outputs: columns >= K, taus past
    S_k and failed problems keep the sentinel; taus by sequential addition; the limits of the table are the model's."""
    m, D, stride = engine, 3, 211
    c, dts, n_segs = loaded_set(D)
    env = make_env(m, D)
    poly = env.alloc_poly(K_CAP, W_CAP)
    h = _raw_load(m, env, poly, device, c, dts, n_segs, m.ACC, stride, WMAX)
    assert (h["status"][K:] == 0x5A).all() and h["status"][:K].tolist() == [0 if S else m.SOLVE_EMPTY for S in S_OF]
    for k in range(stride):
        S = S_OF[k] if k < K else 0
        assert h["n_segs"][k] == (S if S else -77), k
        assert (h["total_time"][k] == SENTINEL) == (S == 0), k
        col, rows = h["taus"][:, k], S + 1 if S else 0
        assert (col[rows:] == SENTINEL).all(), k
        if S:
            same_bits(col[:rows], taus_of(dts[:, k], S), "taus of problem %d" % k)
            same_bits(h["total_time"][k], col[S], "total time of problem %d" % k)
    poly.n, poly.n_wmax = K, WMAX  # (the raw call went round the Python bookkeeping)
    got = poly.limits(MV_LOADED, 0.0, 0.0)
    for k in LIVE[::7]:
        w = LM.traj_limits([c[s, :D, :, k] for s in range(S_OF[k])], dts[:S_OF[k], k], m.ACC, MV_LOADED, 0, 0, REF)
        for key in KEYS:
            same_bits(got[key][:, k], w[key], "%s of problem %d" % (key, k))
        assert (got["exceed"][k], got["valid"][k], got["first_bad"][k]) == (w["exceed"], w["valid"], w["first_bad"]) and w["first_bad"] == s_bad(k), k
    poly.free()
    env.close()


# ------------------------------------------------------------------------------------------------------------- scale
RATIOS = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0]


@functools.lru_cache(maxsize=None)
def ratios_of_set():
    rng = np.random.default_rng(78)
    ri, rf = rng.choice(RATIOS, K), rng.choice(RATIOS, K)
    same = ri == rf
    rf[same] = np.where(ri[same] == 4.0, 0.25, 4.0)
    return ri, rf


def taus_of(dts_k, S):
    return SM.set_time(dts_k[:S])


@functools.lru_cache(maxsize=None)
def scale_models(D, mode):
    c, dts, n_segs = loaded_set(D)
    ri, rf = ratios_of_set()
    return [SCM.scale(taus_of(dts[:, k], S_OF[k]), ri[k], rf[k], mode) if S_OF[k] else None for k in range(K)]


@pytest.mark.parametrize("mode", [SCM.REFERENCE, SCM.ROBUST], ids=["reference", "robust"])
@pytest.mark.parametrize("D", [2, 3])
def test_scale_fills_every_boundary(engine, D, mode):
    """scale(ri, rf): the Lambda, Ts[0 .. S_k] and the total bit for bit, rows past S_k untouched; then one sample at the
    scaled boundaries Ts, bit for bit given the device's tau."""
    m = engine
    c, dts, n_segs = loaded_set(D)
    ri, rf = ratios_of_set()
    env = make_env(m, D, control=JRKxYAW)
    poly = load_into(m, env, env.alloc_poly(K_CAP, W_CAP), c, dts, n_segs, JRKxYAW)
    models = scale_models(D, mode)
    # the _device form on rows filled with a pattern: what it does not own keeps the caller's bytes
    rows_d = env.alloc_lambda_rows(K, WMAX)
    rows_d.fill(FILL)
    d_ri, d_rf = m.DeviceArray(env, K * 8), m.DeviceArray(env, K * 8)
    d_ri.upload(ri)
    d_rf.upload(rf)
    poly.scale_resident(rows_d, d_ri, d_rf, robust=mode == SCM.ROBUST)
    env.synchronize()
    d = rows_d.download()
    h = poly.scale(ri, rf, robust=mode == SCM.ROBUST)
    assert h["Ts"].shape == (WMAX, K) and d["Ts"].shape == (WMAX, K)
    for k, r in enumerate(models):
        n, S = (0, -1) if r is None else (r["lam"].n, S_OF[k])
        if r is None:
            assert d["status"][k] == FILL and d["n_lseg"][k] == FILL_I32, k
            same_bits(d["total"][k], FILL_F64, "device form: total of the failed load %d" % k)
        else:
            assert d["status"][k] == 0 and d["n_lseg"][k] == n, k
            same_bits(d["total"][k], r["total"], "device form: total of problem %d" % k)
            same_bits(d["segs"][:n, :, k], r["lam"].segs, "device form: Lambda segments of problem %d" % k)
            same_bits(d["Ts"][:S + 1, k], r["Ts"], "device form: Ts of problem %d" % k)
        same_bits(d["segs"][n:, :, k], np.full((8 - n, 8), FILL_F64), "device form: segment rows past n_lseg of problem %d" % k)
        same_bits(d["Ts"][S + 1:, k], np.full(WMAX - S - 1, FILL_F64), "device form: Ts past S of problem %d" % k)
    times = np.zeros((K, WMAX))
    for k, r in enumerate(models):
        if r is None:
            assert h["status"][k] == 0 and h["n_lseg"][k] == 0 and h["total"][k] == 0 and not h["Ts"][:, k].any() and not h["segs"][..., k].any(), k
            continue
        S, lam = S_OF[k], r["lam"]
        assert h["status"][k] == r["status"] == 0 and h["n_lseg"][k] == lam.n, k
        same_bits(h["segs"][:lam.n, :, k], lam.segs, "Lambda segments of problem %d" % k)
        assert not h["segs"][lam.n:, :, k].any(), k
        same_bits(h["Ts"][:S + 1, k], r["Ts"], "Ts of problem %d" % k)
        assert not h["Ts"][S + 1:, k].any(), k
        same_bits(h["total"][k], r["total"], "total of problem %d" % k)
        times[k] = r["total"]  # (the columns past S_k repeat the last boundary)
        times[k, :S + 1] = r["Ts"]
    same_bits(poly.info()["total_time"][LIVE], [models[k]["total"] for k in LIVE], "scaled totals")
    raw = poly.tau(times=times)["tau"]
    rows = 4 * D + 3
    got = poly.sample(times=times, form=m.TRAJ_COMMAND, out=np.full((rows, K, WMAX), SENTINEL))["samples"]
    for k, r in enumerate(models):
        if r is None:
            assert (got[:, k] == SENTINEL).all(), k
            continue
        S = S_OF[k]
        taus = taus_of(dts[:, k], S)
        want = np.zeros((rows, WMAX))
        for q in range(WMAX):
            tau, l, ld = r["lam"].clamp_eval(raw[k, q], r["total"], taus[-1])
            want[:, q] = SCM.sample_rows(c[:S, :D, :, k], c[:S, D, :, k], taus, tau, l, ld, times[k, q], True)
        same_rows(got[:, k], want, "samples at Ts of problem %d" % k)
    for b in (rows_d, d_ri, d_rf, poly):
        b.free()
    env.close()


@pytest.mark.parametrize("D", [2, 3])
def test_scale_down_is_decided_by_the_planted_segment(engine, D):
    """scale_down(v_max = 1): only the planted segments break the limit, so max_l, t_lo and t_hi come from them.  With
    c0 = c1 = 0 the velocity's extremum is the root of a linear equation: every candidate is IEEE arithmetic, a segment
    end or not, and all of it is held bit for bit (the cbrt / acos bound of tests/test_gpu_scale.py has no case here)."""
    m = engine
    c, dts, n_segs = loaded_set(D)
    env = make_env(m, D, control=JRKxYAW)
    poly = load_into(m, env, env.alloc_poly(K_CAP, W_CAP), c, dts, n_segs, JRKxYAW)
    rows_d = env.alloc_lambda_rows(K, WMAX)
    rows_d.fill(FILL)
    poly.scale_down_resident(rows_d, v_max=MV_LOADED, a_max=0.0, ri=1.0, rf=1.0, robust=True)
    env.synchronize()
    d = rows_d.download()
    h = poly.scale_down(v_max=MV_LOADED, a_max=0.0, ri=1.0, rf=1.0, robust=True)
    for k in range(K):  # the device form: the host form's values, the caller's bytes where it owns nothing
        S = S_OF[k]
        if S == 0:
            assert d["scaled"][k] == FILL and d["status"][k] == FILL and d["n_lseg"][k] == FILL_I32, k
            same_bits([d["max_l"][k], d["t_lo"][k], d["t_hi"][k], d["total"][k]], [FILL_F64] * 4, "device form: the failed load %d" % k)
            same_bits(d["Ts"][:, k], np.full(WMAX, FILL_F64), "device form: Ts of the failed load %d" % k)
            continue
        for key in ("scaled", "status", "n_lseg", "max_l", "t_lo", "t_hi", "total"):
            same_bits(np.float64(d[key][k]), np.float64(h[key][k]), "host and device form, %s of problem %d" % (key, k))
        n = int(h["n_lseg"][k])
        same_bits(d["segs"][:n, :, k], h["segs"][:n, :, k], "host and device form, Lambda segments of problem %d" % k)
        same_bits(d["segs"][n:, :, k], np.full((8 - n, 8), FILL_F64), "device form: segment rows past n_lseg of problem %d" % k)
        same_bits(d["Ts"][:S + 1, k], h["Ts"][:S + 1, k], "host and device form, Ts of problem %d" % k)
        same_bits(d["Ts"][S + 1:, k], np.full(WMAX - S - 1, FILL_F64), "device form: Ts past S of problem %d" % k)
    late = 0
    for k in range(K):
        S = S_OF[k]
        if S == 0:
            assert h["scaled"][k] == 0 and h["n_lseg"][k] == 0 and not h["Ts"][:, k].any(), k
            continue
        taus = taus_of(dts[:, k], S)
        w = SCM.scale_down([c[s, :D, :, k] for s in range(S)], dts[:S, k], taus, MV_LOADED, 0.0, 1.0, 1.0, SCM.ROBUST)
        assert h["scaled"][k] == w["scaled"] == 1, k
        for key in ("max_l", "t_lo", "t_hi", "total"):
            same_bits(h[key][k], w[key], "%s of problem %d" % (key, k))
        s1 = s_bad(k)
        s2 = s1 if s_bad2(k) is None else s_bad2(k)
        assert taus[s1] <= h["t_lo"][k] <= taus[s1 + 1] and taus[s2] <= h["t_hi"][k] <= taus[s2 + 1], (k, s1, s2)
        assert h["max_l"][k] > 1.4
        late += s1 >= 16
        assert h["status"][k] == w["status"] == 0 and h["n_lseg"][k] == w["lam"].n, k
        same_bits(h["segs"][:w["lam"].n, :, k], w["lam"].segs, "Lambda segments of problem %d" % k)
        same_bits(h["Ts"][:S + 1, k], w["Ts"], "Ts of problem %d" % k)
        assert not h["Ts"][S + 1:, k].any(), k
    assert late >= 5
    rows_d.free()
    poly.free()
    env.close()


# ---------------------------------------------------------------------------------------------------- one long-lived pair
def test_a_long_lived_pair_of_polys_ends_as_a_fresh_one(engine):
    """Two polys of capacity (256, 40): one holds the long so = 2 solve, the other the long load; both go through limits
    and a scale, the first is cleared (clear_lambda), the second keeps its Lambda; then the old set (so = 1, K = 67,
    w_max = 7) is solved into each.  Everything they then return is a fresh poly's, bit for bit: no row of the larger
    layout, and no Lambda, shows through."""
    m, D = engine, 2
    env = make_env(m, D)
    a = solve_long(m, env, D, 2, "given")
    c, dts, n_segs = loaded_set(D)
    b = load_into(m, env, env.alloc_poly(K_CAP, W_CAP), c, dts, n_segs, JRKxYAW)
    ri, rf = ratios_of_set()
    for p in (a, b):
        p.limits(1.0, 1.5, 0.0, all_roots=True)
        p.scale(ri, rf)
        assert p.tau(N=4)["found"][LIVE].all()
    a.clear_lambda()
    wp, n_wp, odts, _ = old_problems(D)
    Ko = wp.shape[2]
    fresh = solve_into(m, env, env.alloc_poly(Ko, wp.shape[1]), wp, n_wp, odts, 1.0, m.ACC)
    want = {"coef": fresh.coefficients(), "taus": fresh.taus(), "info": fresh.info(want_states=True),
            "sample": fresh.sample(N=40, out=np.full((4 * D + 3, Ko, 41), SENTINEL)), "limits": fresh.limits(1.0, 1.5, 0.0, all_roots=True),
            "way": fresh.sample(N=7, form=m.TRAJ_WAYPOINT)}
    assert (fresh.status == 0).sum() > 40
    for name, p in (("solved", a), ("loaded and scaled", b)):
        solve_into(m, env, p, wp, n_wp, odts, 1.0, m.ACC)
        with pytest.raises(m._abi.MplxError):  # no Lambda left
            p.tau(N=4)
        assert np.array_equal(p.status, fresh.status) and np.array_equal(p.n_segs, fresh.n_segs)
        same_bits(p.coefficients(), want["coef"], "%s: coefficients" % name)
        same_bits(p.taus(), want["taus"], "%s: taus" % name)
        info = p.info(want_states=True)
        for key in ("total_time", "effort", "seg_state"):
            same_bits(info[key], want["info"][key], "%s: info %s" % (name, key))
        same_bits(p.sample(N=40, out=np.full((4 * D + 3, Ko, 41), SENTINEL))["samples"], want["sample"]["samples"], "%s: samples" % name)
        same_bits(p.sample(N=7, form=m.TRAJ_WAYPOINT)["samples"], want["way"]["samples"], "%s: waypoint samples" % name)
        lim = p.limits(1.0, 1.5, 0.0, all_roots=True)
        for key in lim:
            assert np.array_equal(np.asarray(lim[key]).view(np.uint8), np.asarray(want["limits"][key]).view(np.uint8)), (name, key)
    for p in (a, b, fresh):
        p.free()
    env.close()
