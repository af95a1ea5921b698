"""Conflicts between trajectories on a common clock (include/mplx_conflict.h, csrc/conflict_kernel.hip) against
tests/conflict_model.py, bit for bit.

The model is fed the device's own positions: sample(times=column) in Command form at i * step - t0[k], a call the other
trajectory tests pin to the reference.  What is compared is everything the conflict kernels add: inclusion, the active
bit, the pair test, charging, the four minima, whatever the tiling and the chunking.

Main fixture: K = 70 (a wave and six lanes), w_max = 6, S = k % 6 (S = 0: failed loads, excluded); loaded segments with
c5 on the quarter grid in [0, 32) (D = 2) / [0, 8) (D = 3), c4 in sixteenths within +-1, c3 in sixteenths within +-0.5,
the rest 0; segment times in quarters from 0.5 to 3; t0 in quarters from -1 to 2; radii from {0.125, 0.25, 0.5};
group = k // 2; step = 0.25, n_steps = 41.  On the model's answer the share of included trajectories with a conflict
must lie in [0.2, 0.8] in both modes, with -1, 0 and positive first steps all present: the comparison is not vacuous."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import conflict_model as CM
from test_gpu_solve import same_bits

pytestmark = pytest.mark.gpu

K, WMAX, STEP, NSTEPS = 70, 6, 0.25, 41
JRKxYAW = 0x17
FILL = 0xAB
FILL_F64 = np.frombuffer(bytes([FILL] * 8), dtype=np.float64)[0]
FILL_I32 = np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0]
MODES = [pytest.param(CM.PARK, id="park"), pytest.param(CM.GONE, id="gone")]


@functools.lru_cache(maxsize=None)
def fixture(D, n=K, seed=0):
    """coeff [5][D + 1][6][n], dts [5][n], n_segs, t0, radius, group, rank."""
    rng = np.random.default_rng(9100 + 10 * D + seed)
    c = np.zeros((WMAX - 1, D + 1, 6, n))
    c[:, :D, 5, :] = rng.integers(0, 4 * (32 if D == 2 else 8), (WMAX - 1, D, n)) / 4.0
    c[:, :D, 4, :] = rng.integers(-16, 17, (WMAX - 1, D, n)) / 16.0
    c[:, :D, 3, :] = rng.integers(-8, 9, (WMAX - 1, D, n)) / 16.0
    dts = rng.integers(2, 13, (WMAX - 1, n)) / 4.0
    n_segs = (np.arange(n) % WMAX).astype(np.int32)
    t0 = rng.integers(-4, 9, n) / 4.0
    radius = rng.choice([0.125, 0.25, 0.5], n)
    group = (np.arange(n) // 2).astype(np.int32)
    rank = rng.integers(0, 5, n).astype(np.int32)
    return c, dts, n_segs, t0, radius, group, rank


def make_set(m, D, n=K, seed=0):
    env = m.EnvMap(D)
    env.set_control(JRKxYAW)
    env.set_v_max(2.0)
    env.set_a_max(1.5)
    c, dts, n_segs = fixture(D, n, seed)[:3]
    poly = env.load_traj(c, dts, n_segs=n_segs, control=JRKxYAW)
    assert (poly.status[n_segs == 0] == m.SOLVE_EMPTY).all() and (poly.status[n_segs > 0] == 0).all()
    return env, poly


def device_positions(sample, n_traj, D, tl):
    """pos [n][K][D] from the device's own Command samples at the local times tl [K][n]."""
    s = sample(np.ascontiguousarray(tl))["samples"]
    return np.ascontiguousarray(s[:D].transpose(2, 1, 0))


def model_of(sample, status, total, D, step, n_steps, mode, t0, radius, group=None, rank=None):
    n = len(status)
    tl = CM.local_times(step, n_steps, t0, n)
    inc = (status == 0) & CM.inputs_ok(n, t0, radius)
    want = CM.conflicts(device_positions(sample, n, D, tl), CM.active_mask(tl, total, mode), radius, inc, group=group, rank=rank)
    want["status"] = (status | np.where(CM.inputs_ok(n, t0, radius), 0, CM.BAD_INPUT)).astype(np.uint8)
    return want, inc


def poly_model(poly, D, mode, t0, radius, group=None, rank=None, step=STEP, n_steps=NSTEPS):
    info = poly.info()
    return model_of(lambda tl: poly.sample(times=tl), info["status"], info["total_time"], D, step, n_steps, mode, t0, radius, group, rank)


def assert_result(res, want, what, pairs=True):
    assert np.array_equal(res.first_step, want["first_step"]), (what, "first_step", res.first_step, want["first_step"])
    assert np.array_equal(res.partner, want["first_partner"]), (what, "partner")
    same_bits(res.min_d2, want["min_d2"], what + ": min_d2")
    assert np.array_equal(res.status, want["status"]), (what, "status")
    if pairs:
        assert np.array_equal(res.pairs, want["pair_first"]), (what, "pair_first")
        assert np.array_equal(res.pairs, res.pairs.T), (what, "pair_first is symmetric")


def not_vacuous(want, inc, what):
    fs = want["first_step"][inc]
    share = float((fs >= 0).mean())
    print("%s: share of included trajectories in conflict %.3f, %d of them later than the first instant" % (what, share, (fs > 0).sum()))
    assert 0.2 <= share <= 0.8, (what, share)
    assert (fs == -1).any() and (fs >= 0).any() and (fs > 0).any(), what


VARIANTS = {"all": (1, 1, 1, 1), "no_t0": (0, 1, 1, 1), "scalar_radius": (1, 0, 1, 1), "no_group": (1, 1, 0, 1), "no_rank": (1, 1, 1, 0),
            "none": (0, 0, 0, 0)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("D", [2, 3])
def test_against_the_model(engine, D, mode):
    m = engine
    env, poly = make_set(m, D)
    _, _, n_segs, t0, radius, group, rank = fixture(D)
    for name, (ut, ur, ug, uk) in VARIANTS.items():
        kw = dict(t0=t0 if ut else None, radius=radius if ur else 0.25, group=group if ug else None, rank=rank if uk else None)
        want, inc = poly_model(poly, D, mode, **kw)
        if name in ("all", "no_rank"):
            not_vacuous(want, inc, "D=%d mode=%d %s" % (D, mode, name))
        res = poly.conflicts(STEP, NSTEPS, park=mode == CM.PARK, want_pairs=True, **kw)
        assert_result(res, want, "host form, " + name)
        assert (res.first_step[n_segs == 0] == -1).all() and np.isinf(res.min_d2[n_segs == 0]).all()
    # the _device form on rows filled with a pattern, five entries and columns longer than K: the same bits as the host
    # twin, and what lies past K keeps the caller's bytes
    P = K + 5
    rows = env.alloc_conflicts(P, want_pairs=True)
    rows.fill(FILL)
    bufs = [m.DeviceArray(env, a.nbytes) for a in (t0, radius, group, rank)]
    for b, a in zip(bufs, (t0, radius, group, rank)):
        b.upload(a)
    poly.conflicts_resident(rows, STEP, NSTEPS, t0=bufs[0], radius=bufs[1], group=bufs[2], rank=bufs[3], park=mode == CM.PARK)
    env.synchronize()
    d = rows.download()
    want, _ = poly_model(poly, D, mode, t0, radius, group, rank)
    host = poly.conflicts(STEP, NSTEPS, t0=t0, radius=radius, group=group, rank=rank, park=mode == CM.PARK, want_pairs=True)
    assert np.array_equal(d["first_step"][:K], host.first_step) and np.array_equal(d["first_partner"][:K], host.partner)
    same_bits(d["min_d2"][:K], host.min_d2, "device form: min_d2")
    assert np.array_equal(d["status"][:K], host.status) and np.array_equal(d["pair_first"][:K, :K], host.pairs)
    assert_result(m.ConflictResult(STEP, d["first_step"][:K], d["first_partner"][:K], d["min_d2"][:K], d["status"][:K], d["pair_first"][:K, :K]),
                  want, "device form")
    assert (d["first_step"][K:] == FILL_I32).all() and (d["first_partner"][K:] == FILL_I32).all() and (d["status"][K:] == FILL).all()
    same_bits(d["min_d2"][K:], np.full(P - K, FILL_F64), "min_d2 past K")
    assert (d["pair_first"][K:, :] == FILL_I32).all() and (d["pair_first"][:K, K:] == FILL_I32).all()
    for b in bufs:
        b.free()
    rows.free()
    poly.free()
    env.close()


@pytest.mark.parametrize("D", [2, 3])
def test_chunking_changes_nothing(engine, D):
    m = engine
    env, poly = make_set(m, D)
    _, _, _, t0, radius, group, rank = fixture(D)
    for mode in (CM.PARK, CM.GONE):
        want, _ = poly_model(poly, D, mode, t0, radius, group, rank)
        for chunk in (0, 1, 7, 41):
            res = poly.conflicts(STEP, NSTEPS, t0=t0, radius=radius, group=group, rank=rank, park=mode == CM.PARK, want_pairs=True,
                                 chunk_steps=chunk)
            assert_result(res, want, "chunk_steps %d mode %d" % (chunk, mode))
    poly.free()
    env.close()


@pytest.mark.parametrize("n,n_steps", [(1, 41), (2, 41), (70, 1), (257, 41)])
def test_small_and_large_shapes(engine, n, n_steps):
    """K = 1 and 2, one instant, and K = 257: one past 64, 128 and 256, any tile edge."""
    m = engine
    D = 2
    if n <= 2:  # (S = k % 6 would make trajectory 0 a failed load: take trajectories 1, 2 of the K = 70 set)
        c, dts, n_segs, t0, radius, group, rank = (a[..., 1:1 + n] for a in fixture(D))
        group = np.arange(n, dtype=np.int32)
        env = m.EnvMap(D)
        env.set_control(JRKxYAW)
        poly = env.load_traj(np.ascontiguousarray(c), np.ascontiguousarray(dts), n_segs=np.ascontiguousarray(n_segs), control=JRKxYAW)
    else:
        env, poly = make_set(m, D, n, seed=1 if n > K else 0)
        _, _, _, t0, radius, group, rank = fixture(D, n, 1 if n > K else 0)
    for mode in (CM.PARK, CM.GONE):
        for rk in (rank, None):
            want, inc = poly_model(poly, D, mode, t0, radius, group, rk, n_steps=n_steps)
            res = poly.conflicts(STEP, n_steps, t0=t0, radius=radius, group=group, rank=rk, park=mode == CM.PARK, want_pairs=True)
            assert_result(res, want, "K=%d n_steps=%d mode=%d" % (n, n_steps, mode))
            if n == 257 and rk is not None:
                not_vacuous(want, inc, "K=257 mode=%d" % mode)
    poly.free()
    env.close()


@pytest.mark.parametrize("D", [2, 3])
def test_scaled_set(engine, D):
    """scale_down(robust=True): positions through getTau, GONE against the scaled total."""
    m = engine
    env, poly = make_set(m, D)
    _, _, n_segs, t0, radius, group, rank = fixture(D)
    down = poly.scale_down(v_max=0.75, a_max=0.5, robust=True)
    assert down["scaled"].sum() >= 10
    info = poly.info()
    assert (info["total_time"][down["scaled"] == 1] > poly.total_time[down["scaled"] == 1]).all()
    n_steps = 61
    for mode in (CM.PARK, CM.GONE):
        want, inc = poly_model(poly, D, mode, t0, radius, group, rank, n_steps=n_steps)
        assert (want["first_step"][inc] >= 0).any() and (want["first_step"][inc] < 0).any()
        res = poly.conflicts(STEP, n_steps, t0=t0, radius=radius, group=group, rank=rank, park=mode == CM.PARK, want_pairs=True)
        assert_result(res, want, "scaled set, mode %d" % mode)
    # n_steps=None covers the scaled totals
    res = poly.conflicts(STEP, t0=t0, radius=radius, park=False)
    n_auto = CM.n_steps_for(STEP, t0, info["total_time"], info["status"] == 0)
    want, _ = poly_model(poly, D, CM.GONE, t0, radius, n_steps=n_auto)
    assert_result(res, want, "scaled set, automatic n_steps", pairs=False)
    assert (n_auto - 1) * STEP >= (t0 + info["total_time"])[info["status"] == 0].max() > (n_auto - 2) * STEP
    poly.free()
    env.close()


def test_bad_inputs_are_excluded(engine):
    m = engine
    D = 2
    env, poly = make_set(m, D)
    _, _, n_segs, t0, radius, group, rank = fixture(D)
    t0, radius = t0.copy(), radius.copy()
    t0[7], t0[13], radius[19], radius[25], radius[31] = np.nan, np.inf, -0.25, np.nan, np.inf
    bad = [7, 13, 19, 25, 31]
    assert all(n_segs[k] > 0 for k in bad)
    for mode in (CM.PARK, CM.GONE):
        want, inc = poly_model(poly, D, mode, t0, radius, group, rank)
        assert not inc[bad].any()
        res = poly.conflicts(STEP, NSTEPS, t0=t0, radius=radius, group=group, rank=rank, park=mode == CM.PARK, want_pairs=True)
        assert_result(res, want, "bad inputs, mode %d" % mode)
        assert (res.status[bad] == m.CONFLICT_BAD_INPUT).all() and (res.first_step[bad] == -1).all() and (res.partner[bad] == -1).all()
        assert np.isinf(res.min_d2[bad]).all() and (res.pairs[bad] == -1).all() and (res.pairs[:, bad] == -1).all()
        assert (res.status[n_segs == 0] == m.SOLVE_EMPTY).all() and not (res.partner[:, None] == np.array(bad)[None, :]).any()
    # a negative scalar radius excludes everybody
    res = poly.conflicts(STEP, NSTEPS, radius=-1.0)
    assert (res.status[n_segs > 0] == m.CONFLICT_BAD_INPUT).all() and (res.first_step == -1).all()
    poly.free()
    env.close()


def test_action_chains_and_search_result(engine):
    """mplx_traj_conflicts on a context without a map against the model fed by traj_sample, and equal to
    MultiSearchResult.conflicts on the same chains."""
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    m = engine
    env, _, _ = corridor_env(m)
    starts, goals = corridor_queries(m)
    multi = env.search_many(starts, goals, eps=1.0, delta=10.0, capacity=1 << 16)
    assert multi.found == [True] * 3
    paths = [multi.path(q) for q in range(3)]
    Q = 3
    H = max(len(p[1]) for p in paths) + 2
    # a fourth chain that is empty and a fifth with a bad action: both excluded
    S = np.zeros((env.n_fields, Q + 2))
    A = np.full((H, Q + 2), -1, np.int32)
    for q, (s0, act) in enumerate(paths):
        S[:, q], A[:len(act), q] = s0, act
    S[:, 4], A[:3, 4] = paths[0][0], [0, 99, 0]
    bare = m.EnvMap(2)  # no map
    bare.set_control(m.ACC)
    bare.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    bare.set_v_max(1.0)
    bare.set_a_max(1.0)
    bare.set_dt(1.0)
    t0 = np.array([0.0, 1.5, -2.0, 0.0, 0.0])
    radius = np.array([0.25, 0.5, 0.25, 0.5, 0.5])
    step = 0.5
    info = bare.traj_info(S, A)
    assert info["status"].tolist() == [0, 0, 0, m.TRAJ_EMPTY, m.TRAJ_BAD_ACTION]
    n_auto = CM.n_steps_for(step, t0, info["total_time"], info["status"] == 0)
    for mode in (CM.PARK, CM.GONE):
        for rk in (None, np.array([2, 1, 0, 0, 0], np.int32)):
            want, inc = model_of(lambda tl: bare.traj_sample(S, A, times=tl), info["status"], info["total_time"], 2, step, n_auto, mode,
                                 t0, radius, None, rk)
            assert inc.tolist() == [True, True, True, False, False]
            res = bare.traj_conflicts(S, A, step, t0=t0, radius=radius, rank=rk, park=mode == CM.PARK, want_pairs=True)
            assert_result(res, want, "chains, mode %d" % mode)
            assert res.first_step[2] >= 0 or rk is not None  # the way back meets query 0 head-on
            # the search result's own method, on the context that holds the map: the first Q entries
            r3 = multi.conflicts(step, n_steps=n_auto, t0=t0[:Q], radius=radius[:Q], rank=None if rk is None else rk[:Q],
                                 park=mode == CM.PARK, want_pairs=True)
            assert np.array_equal(r3.first_step, res.first_step[:Q]) and np.array_equal(r3.partner, res.partner[:Q])
            same_bits(r3.min_d2, res.min_d2[:Q], "MultiSearchResult.conflicts: min_d2")
            assert np.array_equal(r3.pairs, res.pairs[:Q, :Q]) and np.array_equal(r3.status, res.status[:Q])
    # the _device form
    rows = bare.alloc_conflicts(Q + 2, want_pairs=True)
    bufs = [m.DeviceArray(bare, a.nbytes) for a in (S, A, t0, radius)]
    for b, a in zip(bufs, (S, A, t0, radius)):
        b.upload(a)
    bare.traj_conflicts_resident(bufs[0], bufs[1], rows, H, step, n_auto, t0=bufs[2], radius=bufs[3], park=True)
    bare.synchronize()
    host = bare.traj_conflicts(S, A, step, n_steps=n_auto, t0=t0, radius=radius, park=True, want_pairs=True)
    d = rows.download()
    assert np.array_equal(d["first_step"], host.first_step) and np.array_equal(d["first_partner"], host.partner)
    same_bits(d["min_d2"], host.min_d2, "chains, device form")
    assert np.array_equal(d["pair_first"], host.pairs) and np.array_equal(d["status"], host.status)
    for b in bufs:
        b.free()
    rows.free()
    multi.free()
    bare.close()
    env.close()


def test_argument_errors_and_state(engine):
    m = engine
    L, A = m._abi.lib(), m._abi
    env, poly = make_set(m, 2)
    n = poly.n
    out = {"fs": np.zeros(n, np.int32), "pairs": np.zeros((n, n), np.int32)}

    def call(fn, h, *set_, null_in=False, null_out=False, **kw):
        i, o = A.ConflictIn(), A.ConflictOut()
        i.step, i.n_steps, i.mode, i.radius_all = 0.25, 4, CM.PARK, 0.25
        o.first_step = out["fs"].ctypes.data
        for k, v in kw.items():
            setattr(o if k in ("pair_first", "pair_stride") else i, k, v)
        return fn(h, *set_, None if null_in else C.byref(i), None if null_out else C.byref(o))

    assert call(L.mplx_poly_conflicts, poly._h) == A.OK  # (host rows: only the host form may be let through to a launch)
    for fn in (L.mplx_poly_conflicts, L.mplx_poly_conflicts_device):
        assert fn(None, None, None) == A.ERR_ARG
        assert call(fn, poly._h, null_in=True) == A.ERR_ARG and call(fn, poly._h, null_out=True) == A.ERR_ARG
        for bad in (dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(step=float("inf")), dict(n_steps=0), dict(mode=2),
                    dict(mode=-1), dict(chunk_steps=-1), dict(pair_first=out["pairs"].ctypes.data, pair_stride=n - 1)):
            assert call(fn, poly._h, **bad) == A.ERR_ARG, (fn, bad)
    env.synchronize()
    fresh = env.alloc_poly(4, 3)  # nothing solved or loaded
    assert call(L.mplx_poly_conflicts, fresh._h) == A.ERR_STATE and call(L.mplx_poly_conflicts_device, fresh._h) == A.ERR_STATE
    fresh.free()
    poly.free()
    env.close()

    # chains: a context without params / controls; K == 0 is a no-op
    bare = m.EnvMap(2)
    starts, acts = np.zeros((bare.n_fields, 2)), np.zeros((3, 2), np.int32)
    s = A.TrajSet()
    s.starts, s.n_starts, s.start_stride, s.actions, s.n_traj, s.horizon, s.action_stride = starts.ctypes.data, 2, 2, acts.ctypes.data, 2, 3, 2
    for fn in (L.mplx_traj_conflicts, L.mplx_traj_conflicts_device):
        assert fn(None, None, None, None) == A.ERR_ARG
        assert call(fn, bare._ctx, None) == A.ERR_ARG
        assert call(fn, bare._ctx, C.byref(s), step=0.0) == A.ERR_ARG
        assert call(fn, bare._ctx, C.byref(s)) == A.ERR_STATE  # no controls
    bare.set_control(m.ACC)
    bare.set_dt(1.0)
    bare.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    bare._flush()  # (the setters above are lazy; the raw calls below do not go through EnvMap)
    assert call(L.mplx_traj_conflicts, bare._ctx, C.byref(s)) == A.OK
    s.n_traj, s.n_starts = 0, 1  # (n_starts is 1 or n_traj: include/mplx_traj.h)
    out["fs"][:] = 77
    assert call(L.mplx_traj_conflicts, bare._ctx, C.byref(s)) == A.OK and (out["fs"] == 77).all()
    bare.close()


def test_stagger_four_robot_crossing(engine):
    """search.stagger on four robots that all pass (4, 4) at t = 4, against the model's loop around the device's samples."""
    m = engine
    D = 2
    env = m.EnvMap(D)
    env.set_control(JRKxYAW)
    c = np.zeros((1, D + 1, 6, 4))
    c[0, :D, 5, :] = [[0, 4, 0, 8], [4, 0, 0, 0]]     # starts: two along the axes, two along the diagonals
    c[0, :D, 4, :] = [[1, 0, 1, -1], [0, 1, 1, 1]]    # velocities; starts and ends are all at least 4 apart
    poly = env.load_traj(c, np.full((1, 4), 8.0), control=JRKxYAW)
    assert (poly.status == 0).all()
    info = poly.info()

    def positions_for(mode):
        def positions(t0):
            n = CM.n_steps_for(STEP, t0, info["total_time"], info["status"] == 0)
            tl = CM.local_times(STEP, n, t0, 4)
            return device_positions(lambda t: poly.sample(times=t), 4, D, tl), CM.active_mask(tl, info["total_time"], mode)
        return positions

    for park, rank, rounds_max in ((False, None, 64), (True, None, 64), (False, np.array([0, 0, 1, 2], np.int32), 5)):
        mode = CM.PARK if park else CM.GONE
        w_t0, w_ok, w_rounds = CM.stagger(positions_for(mode), 4, STEP, 0.5, np.ones(4, bool), rank=rank, max_rounds=rounds_max)
        t0, ok, rounds = m.stagger(poly, STEP, 0.5, rank=rank, park=park, max_rounds=rounds_max)
        print("stagger park=%s rank=%s: t0 %s resolved %s rounds %d" % (park, rank, t0, ok, rounds))
        same_bits(t0, w_t0, "stagger: t0")
        assert np.array_equal(ok, w_ok) and rounds == w_rounds
        if rank is None:
            assert ok.all() and t0[0] == 0.0 and (np.diff(t0) > 0).all() and 1 < rounds < 64
        else:
            assert not ok[0] and not ok[1] and rounds == 5  # equal ranks move in lockstep
    poly.free()
    env.close()
