"""Polynomial trajectory sets against a reservation table (include/mplx_reserve_poly.h, csrc/reserve_poly_kernel.hip)
against tests/reserve_poly_model.py, bit for bit: hit, status and n_hit.

The model is fed the table Reservations.positions() returns and the device's own positions of the problems:
sample(times=column) in Command form at i * step - t_start[k], a call the other trajectory tests pin to the reference.
What is compared is everything the kernel adds: exclusion, the horizon, the instants of a problem, the pair test, the
minimum.  Inputs: tests/reserve_poly_cases.py (random_case: the share of problems with a hit and the presence of -2 are
verified on the CPU, tests/test_reserve_poly_model.py; hand_case: one problem per rule, expected hits written out).
Sizes: K in {1, 63, 65} (under, at and over a wave of problems is of no concern to a wave-per-problem kernel, over 64 is a
second workgroup row of the host rows), B in {0, 1, 64, 65, 257} (no tile, one lane, a full tile, a tile and a lane, past
the kKeep = 4 tiles whose radius sums stay in registers)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded (see tests/test_gpu_traj.py)

import reserve_poly_cases as RC
import reserve_poly_model as RPM

pytestmark = pytest.mark.gpu

JRKxYAW = 0x17
FILL = 0xAB
FILL_I64 = np.frombuffer(bytes([FILL] * 8), dtype=np.int64)[0]


def make_env(m, D):
    """Parameters, controls and an all-free map: the check reads none of them, the fill of an EMPTY table (K == 0 action
    chains) wants parameters and controls."""
    env = m.EnvMap(D)
    env.setMap([0.0] * D, [8] * D, np.zeros(8 ** D, np.int8), 1.0)
    env.set_control(JRKxYAW)
    env.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], D, yaw_rates=[0.0]))
    env.set_v_max(2.0)
    env.set_a_max(1.5)
    env.set_dt(1.0)
    return env


def load(env, m, trajs):
    c, dts, n_segs = trajs
    poly = env.load_traj(c, dts, n_segs=n_segs, control=JRKxYAW)
    assert (poly.status[n_segs == 0] == m.SOLVE_EMPTY).all() and (poly.status[n_segs > 0] == 0).all()
    return poly


def make_table(env, m, case, park):
    """(Reservations, the PolyTrajSet it was filled from or None)."""
    B = case["res"][1].shape[1]
    if B == 0:
        empty = (np.zeros((env.n_fields, 0)), np.zeros((1, 0), np.int32))
        return env.alloc_reservations(empty, case["step"], n_steps=case["n_steps"], radius=0.25, park=park), None
    rp = load(env, m, case["res"])
    return env.alloc_reservations(rp, case["step"], n_steps=case["n_steps"], t0=case["t0"], radius=case["r_b"], group=case["group"],
                                  park=park), rp


def model_of(poly, D, case, table, radius=None, ignore="case"):
    """The model's (hit, status, n_hit) for the candidates `poly` with the device's own positions."""
    K, n = poly.n, case["n_steps"]
    info = poly.info()
    ts = case["t_start"]
    with np.errstate(invalid="ignore"):
        tl = np.arange(n)[None, :] * np.float64(case["step"]) - ts[:, None]
    pos = poly.sample(times=np.ascontiguousarray(np.where(np.isfinite(tl), tl, 0.0)))["samples"][:D]  # [D][K][n]
    return RPM.check(info["status"], info["n_segs"], info["total_time"], ts, case["radius"] if radius is None else radius,
                     case["ignore"] if isinstance(ignore, str) else ignore, case["step"], table,
                     lambda k, i, t: pos[:, k, i])


def table_dict(res, D):
    if res.n == 0:
        return {"pos": np.zeros((res.n_steps, D, 0)), "active": np.zeros((res.n_steps, 0), np.uint8), "included": np.zeros(0, np.uint8),
                "radius": np.zeros(0), "group": np.zeros(0, np.int32)}
    return res.positions()


def assert_same(got, want, what):
    hit, status, n_hit = want
    assert np.array_equal(got["hit"], hit), (what, "hit", got["hit"], hit)
    assert np.array_equal(got["status"], status), (what, "status")
    assert got["n_hit"] == n_hit, (what, "n_hit", got["n_hit"], n_hit)
    some = hit >= 0
    assert np.array_equal(got["instant"], np.where(some, hit >> 32, -1)) and np.array_equal(got["partner"], np.where(some, hit & 0xffffffff, -1))


@pytest.mark.parametrize("B", [0, 1, 64, 65, 257])
@pytest.mark.parametrize("K", [1, 63, 65])
@pytest.mark.parametrize("D", [2, 3])
def test_against_the_model(engine, D, K, B):
    m = engine
    env = make_env(m, D)
    case = RC.random_case(D, K, B)
    poly = load(env, m, case["cand"])
    for park in (False, True):
        res, rp = make_table(env, m, case, park)
        table = table_dict(res, D)
        want = model_of(poly, D, case, table)
        got = res.check_poly(poly, case["t_start"], case["radius"], case["ignore"])
        assert_same(got, want, "D=%d K=%d B=%d park=%d" % (D, K, B, park))
        if B == 0:
            assert ((got["hit"] == -1) | (got["hit"] == -2)).all()
        # a scalar radius, nobody ignored
        want = model_of(poly, D, case, table, radius=0.25, ignore=None)
        assert_same(res.check_poly(poly, case["t_start"], 0.25), want, "scalar radius")
        res.free()
        if rp is not None:
            rp.free()
    poly.free()
    env.close()


@pytest.mark.parametrize("D", [2, 3])
def test_the_random_case_and_the_device_twin(engine, D):
    """K = B = 65: the share of hits is the one verified on the CPU (the device's positions give the same hits as the
    host's there: every input is exactly representable); the _device form on rows filled with a pattern and five
    entries longer than K gives the same bits as the host twin, adds to n_hit, and leaves what lies past K alone."""
    m = engine
    env = make_env(m, D)
    K = 65
    case = RC.random_case(D, K, 65)
    poly = load(env, m, case["cand"])
    res, rp = make_table(env, m, case, False)
    want = model_of(poly, D, case, res.positions())
    share = want[2] / float(K)
    print("D=%d: share of problems with a hit %.3f, %d past the horizon" % (D, share, (want[0] == -2).sum()))
    assert 0.2 <= share <= 0.8 and (want[0] == -2).any()
    host = res.check_poly(poly, case["t_start"], case["radius"], case["ignore"])
    assert_same(host, want, "host twin")
    P = K + 5
    rows = {"t": case["t_start"], "r": case["radius"], "g": case["ignore"], "hit": np.full(P, FILL_I64), "st": np.full(P, FILL, np.uint8),
            "n": np.array([1000], np.int64)}
    bufs = {k: m.DeviceArray(env, a.nbytes) for k, a in rows.items()}
    for k, a in rows.items():
        bufs[k].upload(a)
    res.check_poly_resident(poly, bufs["t"], bufs["r"], bufs["g"], hit=bufs["hit"], status=bufs["st"], n_hit=bufs["n"])
    res.check_poly_resident(poly, bufs["t"], bufs["r"], bufs["g"], n_hit=bufs["n"])  # every other output absent
    env.synchronize()
    hit, st, n = bufs["hit"].download(np.int64, (P,)), bufs["st"].download(np.uint8, (P,)), bufs["n"].download(np.int64, (1,))
    assert np.array_equal(hit[:K], host["hit"]) and np.array_equal(st[:K], host["status"]) and n[0] == 1000 + 2 * host["n_hit"]
    assert (hit[K:] == FILL_I64).all() and (st[K:] == FILL).all()
    for b in bufs.values():
        b.free()
    for x in (res, rp, poly):
        x.free()
    env.close()


@pytest.mark.parametrize("park", [False, True])
def test_hand_case(engine, park):
    """One problem per rule (tests/reserve_poly_cases.py:hand_case): windows of 0, 1, 64 and 65 instants, a first and a
    last instant exactly on tl = 0 and tl = total, a negative t_start, the horizon (exactly on it: checked; one instant
    past: -2), a touching pair, reservations PARK and GONE, excluded, and of the ignored group, a NaN t_start, a
    negative radius, a problem with a set status.  The expected hits are written out there; the model agrees."""
    m = engine
    env = make_env(m, 2)
    case = RC.hand_case(park)
    poly = load(env, m, case["cand"])
    res, rp = make_table(env, m, case, park)
    table = res.positions()
    assert table["status"][6] == m.CONFLICT_BAD_INPUT and not table["included"][5] and not table["included"][6]
    got = res.check_poly(poly, case["t_start"], case["radius"], case["ignore"])
    assert np.array_equal(got["hit"], case["hit"]), (got["hit"], case["hit"])
    assert np.array_equal(got["status"], case["status"]) and got["n_hit"] == int((case["hit"] != -1).sum())
    assert_same(got, model_of(poly, 2, case, table), "hand case")
    for k, n in ((0, 64), (1, 65), (3, 0), (4, 1)):
        assert len(RPM.instants(case["step"], case["n_steps"], case["t_start"][k], case["cand"][1][0, k])) == n
    for x in (res, rp, poly):
        x.free()
    env.close()


@pytest.mark.parametrize("robust", [True, False])
@pytest.mark.parametrize("D", [2, 3])
def test_a_set_with_a_lambda(engine, D, robust):
    """scale(2, 0.5): the instants run to the SCALED total and the positions are the Lambda's."""
    m = engine
    env = make_env(m, D)
    K = 63
    case = RC.random_case(D, K, 65, seed=1)
    case["n_steps"] = 90
    poly = load(env, m, case["cand"])
    plain_total = poly.info()["total_time"].copy()
    h = poly.scale(2.0, 0.5, robust=robust)
    ok = case["cand"][2] > 0
    assert (h["status"][ok] == 0).all()
    total = poly.info()["total_time"]
    assert (total[ok] != plain_total[ok]).all()
    res, rp = make_table(env, m, case, False)
    want = model_of(poly, D, case, res.positions())
    assert (want[0] >= 0).sum() >= 10 and (want[0] == -1).any()
    assert_same(res.check_poly(poly, case["t_start"], case["radius"], case["ignore"]), want, "lambda, robust=%s" % robust)
    for x in (res, rp, poly):
        x.free()
    env.close()


@pytest.mark.parametrize("D", [2, 3])
def test_pinned_by_conflicts_of_one_set(engine, D):
    """Needs no new model: candidates and reservations loaded into ONE PolyTrajSet, conflicts(GONE, want_pairs=True) --
    hit[k] = min over the reserved b of (pair_first[k][b] << 32 | b).  The table is long enough for every candidate
    (the merged set knows no horizon) and filled GONE; every candidate is a group of its own and ignores nobody."""
    m = engine
    env = make_env(m, D)
    K, B = 65, 65
    case = RC.random_case(D, K, B)
    case["n_steps"] = 120
    poly = load(env, m, case["cand"])
    res, rp = make_table(env, m, case, False)
    got = res.check_poly(poly, case["t_start"], case["radius"])
    assert not (got["hit"] == -2).any() and (got["hit"] >= 0).sum() >= 10 and (got["hit"] == -1).any()
    (c, dts, ns), (rc, rd, rs) = case["cand"], case["res"]
    merged = load(env, m, (np.concatenate([c, rc], axis=3), np.concatenate([dts, rd], axis=1), np.concatenate([ns, rs])))
    conf = merged.conflicts(case["step"], case["n_steps"], t0=np.concatenate([case["t_start"], case["t0"]]),
                            radius=np.concatenate([case["radius"], case["r_b"]]),
                            group=np.concatenate([1000 + np.arange(K), case["group"]]).astype(np.int32), park=False, want_pairs=True)
    want = RPM.from_pair_first(conf.pairs, range(K), range(K, K + B))
    assert np.array_equal(got["hit"], want), (got["hit"], want)
    for x in (res, rp, poly, merged):
        x.free()
    env.close()


def test_errors(engine):
    m = engine
    A = m._abi
    env = make_env(m, 2)
    case = RC.random_case(2, 9, 1)
    poly = load(env, m, case["cand"])
    res, rp = make_table(env, m, case, True)

    def code(fn):
        with pytest.raises(A.MplxError) as e:
            fn()
        return e.value.code

    ts = np.zeros(9)
    i, o = A.ReservePolyIn(), A.ReservePolyOut()
    i.t_start = ts.ctypes.data
    lib = A.lib()
    fresh = C.c_void_p()
    A.check(env._ctx, lib.mplx_reserve_create(env._ctx, C.byref(fresh)))
    assert code(lambda: A.check(env._ctx, lib.mplx_reserve_check_poly(fresh, poly._h, C.byref(i), C.byref(o)))) == A.ERR_STATE  # before a fill
    lib.mplx_reserve_destroy(fresh)
    assert code(lambda: A.check(env._ctx, lib.mplx_reserve_check_poly(res._res, None, C.byref(i), C.byref(o)))) == A.ERR_ARG
    assert code(lambda: A.check(env._ctx, lib.mplx_reserve_check_poly(res._res, poly._h, None, C.byref(o)))) == A.ERR_ARG
    unsolved = m.PolyTrajSet(env, 4, 3)
    assert code(lambda: A.check(env._ctx, lib.mplx_reserve_check_poly(res._res, unsolved._h, C.byref(i), C.byref(o)))) == A.ERR_STATE
    unsolved.free()
    other = make_env(m, 2)
    theirs = load(other, m, case["cand"])
    assert code(lambda: A.check(env._ctx, lib.mplx_reserve_check_poly(res._res, theirs._h, C.byref(i), C.byref(o)))) == A.ERR_ARG
    theirs.free()
    other.close()
    A.check(env._ctx, lib.mplx_reserve_check_poly(res._res, poly._h, C.byref(i), C.byref(o)))  # every output absent
    for x in (res, rp, poly):
        x.free()
    env.close()
