"""The ellipsoid body against a point cloud (include/mplx_body.h, body_kernel.hip, search.Body, EnvMap.search(body=)) on
the device, against tests/body_model.py.  Every comparison is bit for bit."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import body_cases as BC
import body_model as BM
from test_gpu_open import corridor_env
from test_gpu_table import bits, upload
from test_multi import corridor_queries

pytestmark = pytest.mark.gpu

PAT64 = np.int64(0x5A5A5A5A5A5A5A5A)


def make_body(env, r, h, g=BC.G, mct=0.0, mult=None):
    """EnvMap.alloc_body with min_cos_tilt given as the number itself; mult: MPLX_BODY_CELL_MULT, read at the create."""
    if mult:
        os.environ["MPLX_BODY_CELL_MULT"] = str(mult)
    try:
        body = env.alloc_body(r, h, g)
    finally:
        os.environ.pop("MPLX_BODY_CELL_MULT", None)
    body.set_shape(r, h, g, min_cos_tilt=mct)
    return body


def free_env(m, dim, control, U, dt=BC.DT):
    """Parameters and controls on an all-free map (the check reads no map cell)."""
    env = m.EnvMap(dim)
    env.setMap([0.0] * dim, [8] * dim, np.zeros(8 ** dim, np.int8), 1.0)
    env.set_control(control)
    env.set_u(U)
    env.set_v_max(3.0)
    env.set_a_max(3.0)
    env.set_dt(dt)
    return env


def expected_cells(pts, edge):
    """(included, origin, dims, cell of every point) as include/mplx_body.h's grid bins them, from the edge in force."""
    pts = np.asarray(pts, dtype=np.float64)
    D = pts.shape[1]
    inc = np.isfinite(pts).all(axis=1)
    if not inc.any():
        return inc, np.zeros(3), np.ones(3, np.int64), np.full(len(pts), -1, np.int64)
    lo, hi = pts[inc].min(axis=0), pts[inc].max(axis=0)
    dims = np.ones(3, np.int64)
    dims[:D] = ((hi - lo) / np.float64(edge)).astype(np.int64) + 1
    cell = np.full(len(pts), -1, np.int64)
    if dims.prod() == 1:
        cell[inc] = 0
    else:
        ax = ((pts[inc] - lo) / np.float64(edge)).astype(np.int64)
        c = np.zeros(int(inc.sum()), np.int64)
        for d in range(D - 1, -1, -1):
            c = c * dims[d] + ax[:, d]
        cell[inc] = c
    origin = np.zeros(3)
    origin[:D] = lo
    return inc, origin, dims, cell


# ------------------------------------------------------------------------------------------------------------ binning
@pytest.mark.parametrize("dim,n,far", [(3, 0, False), (3, 1, False), (3, 257, False), (3, 4097, False), (2, 4097, False),
                                       (3, 4097, True), (2, 257, True)],
                         ids=["3d-0", "3d-1", "3d-257", "3d-4097", "2d-4097", "3d-4097-doubling", "2d-257-doubling"])
def test_binning(engine, dim, n, far):
    m = engine
    env = free_env(m, dim, m.ACC, m.workloads.grid_controls([-1.0, 0.0, 1.0], dim))
    r, h = 0.25, 0.125
    rng = np.random.default_rng(n + dim)
    pts = rng.uniform(0.0, 8.0, size=(n, dim))
    if n >= 257:
        pts[3, 0], pts[17, dim - 1], pts[200, 1], pts[201] = np.nan, np.inf, -np.inf, np.nan  # excluded
    if far:
        pts[5], pts[6] = 3.0e6, -1.0e6  # a box of 4e6 m: 1.6e7 cells per axis at the automatic edge
    body = make_body(env, r, h)
    gen0 = body.generation
    body.fill(pts)
    sh = body.shape()
    auto = BC.auto_edge(r, h)
    assert sh["n"] == n and sh["generation"] == gen0 + 1
    # the edge: the automatic one, doubled until the box needs at most 2^22 cells -- and no further
    k = round(math.log2(sh["edge"] / auto))
    assert sh["edge"] == auto * 2.0 ** k and (k > 0) == far
    inc, origin, dims, cell = expected_cells(pts, sh["edge"])
    assert sh["n_excluded"] == n - inc.sum() == (4 if n >= 257 else 0)
    assert sh["cells"].tolist() == dims.tolist() and dims.prod() <= 1 << 22
    if inc.any():
        assert np.array_equal(bits(sh["origin"]), bits(origin))
    if far:
        assert expected_cells(pts, sh["edge"] / 2.0)[2].prod() > 1 << 22
    cop, start = body.cells()
    assert np.array_equal(cop, cell)  # every included point in the cell its coordinates give, the excluded in none
    assert start[0] == 0 and np.array_equal(np.diff(start), np.bincount(cell[inc], minlength=int(dims.prod())))
    assert start[-1] == inc.sum()
    if n >= 257:
        assert (np.diff(start) > 1).any() or far
    # a new shape bins the kept points again; the generation stays
    body.set_shape(2 * r, 2 * h)
    sh2 = body.shape()
    assert sh2["generation"] == sh["generation"] and sh2["n"] == n
    inc2, _, dims2, cell2 = expected_cells(pts, sh2["edge"])
    cop2, start2 = body.cells()
    assert sh2["cells"].tolist() == dims2.tolist() and np.array_equal(cop2, cell2)
    body.free()
    env.close()


# --------------------------------------------------------------------------------------------------------- list check
def run_list_case(m, name, mult=None, refill=None):
    """Case `name` of tests/body_cases.py on the device.  Returns (case, hit, cost, action, count, n_blocked) downloaded."""
    c = BC.list_case(name)
    dim, S, n, n_alloc = c["dim"], c["S"], c["n"], c["n_alloc"]
    env = free_env(m, dim, getattr(m, c["control"]), c["U"])
    body = make_body(env, c["r"], c["h"], BC.G, c["mct"], mult)
    if refill is None:
        body.fill(c["cloud"])
    else:
        refill(env, body, c)
    N = n_alloc * S
    L = m.Lists(env, n_alloc, c["nU"], want_state=False, stride=S)
    L.count.upload(c["count"])
    L.action.upload(c["action"])
    L.cost.upload(c["cost"])
    fr = m.TableFrontier(env, n_alloc)
    fr.id.upload(np.concatenate([c["parent_id"], np.zeros(n_alloc - n, np.int32)]))
    fr.state.upload(c["pst"])
    d_hit = upload(env, m, np.full(N, PAT64, np.int64))
    d_nb = upload(env, m, np.array([5], np.int64))
    body.check(fr, L, n, c["n_samp"], hit=d_hit, n_blocked=d_nb)
    env.synchronize()
    got = (d_hit.download(np.int64, (N,)), L.cost.download(np.float64, (N,)), L.action.download(np.int32, (N,)),
           L.count.download(np.int32, (n_alloc,)), int(d_nb.download(np.int64, (1,))[0]))
    # a second call: the blocked entries are +inf now, nothing new is blocked
    body.check(fr, L, n, c["n_samp"], hit=d_hit, n_blocked=d_nb)
    env.synchronize()
    again = (d_hit.download(np.int64, (N,)), int(d_nb.download(np.int64, (1,))[0]))
    sh = body.shape()
    for b in (d_hit, d_nb, fr, L, body):
        b.free()
    env.close()
    return c, got, again, sh


def assert_list_case(c, got, again):
    S, n = c["S"], c["n"]
    hit, cost, action, count, nb = got
    looked, want_hit = c["looked"], c["want_hit"]
    kinds = {"attitude" if (x & 0xffffffff) == BM.BAD_ATTITUDE else "point" if x >= 0 else "none" for x in want_hit[looked]}
    print("case %s: looked %d blocked %d (%.2f) kinds %s" % (c["name"], looked.sum(), c["want_nb"], c["frac"], sorted(kinds)))
    assert 0.10 <= c["frac"] <= 0.90, c["frac"]  # (on the model's output: at least 10 % blocked, at least 10 % not)
    assert np.array_equal(hit[:n * S], want_hit), np.nonzero(hit[:n * S] != want_hit)[0][:8]
    assert np.all(hit[n * S:] == PAT64)                                   # rows past n_nodes
    assert np.array_equal(bits(cost[:n * S]), bits(c["want_cost"]))       # +inf where blocked, every other byte kept
    assert np.array_equal(bits(cost[n * S:]), bits(c["cost"][n * S:]))
    assert np.array_equal(action, c["action"]) and np.array_equal(count, c["count"])
    assert nb == 5 + c["want_nb"]
    assert again[1] == 5 + c["want_nb"] and np.all(again[0][:n * S] == -1)


# (case, forced multiple of the cell edge): every case at the automatic edge, b and c also at 2x and 7x -- the same bytes
LIST_RUNS = [(k, None) for k in "abcdefg"] + [("b", 2), ("b", 7), ("c", 2), ("c", 7)]


@pytest.mark.parametrize("name,mult", LIST_RUNS, ids=["%s-x%s" % (k, mu or 1) for k, mu in LIST_RUNS])
def test_list_check_equals_the_model(engine, name, mult):
    c, got, again, sh = run_list_case(engine, name, mult)
    assert sh["edge"] >= BC.auto_edge(c["r"], c["h"]) * (mult or 1)
    if "edge" in BC.LIST_CASES[name][-1]:
        assert sh["edge"] == BC.auto_edge(c["r"], c["h"], mult or 1) and not sh["origin"].any()  # the boundary points sit on boundaries
    assert_list_case(c, got, again)
    want_hit = c["want_hit"]
    if name in "bcdf":
        # row 0 stands still at a dyadic position: under its zero control the point r beside it is ON the surface at
        # sample 0 (index 0), its neighbour one ulp further out (index 1) is not
        zero = int(np.nonzero(~c["U"][:, :c["dim"]].any(axis=1))[0][0])
        assert want_hit[zero] == 0
    if name == "g":
        low = want_hit[c["looked"]] & 0xffffffff
        assert (low == BM.BAD_ATTITUDE).sum() > 50 and ((want_hit[c["looked"]] >= 0) & (low != BM.BAD_ATTITUDE)).any()
    if name == "f":
        # yaw must not enter: the same lists with every parent's yaw and every control's yaw rate changed
        c2 = dict(c, pst=c["pst"].copy(), U=c["U"].copy())
        c2["pst"][4 * c["dim"]] += 0.7
        c2["U"][:, c["dim"]] *= -2.0
        BC._cache["f-yaw"] = c2
        BC.LIST_CASES["f-yaw"] = BC.LIST_CASES["f"]
        try:
            _, got2, again2, _ = run_list_case(engine, "f-yaw")
        finally:
            del BC._cache["f-yaw"], BC.LIST_CASES["f-yaw"]
        assert_list_case(c, got2, again2)


def test_fill_map_equals_fill_of_the_cloud(engine):
    """A map with about a hundred occupied cells: fill_map bins what fill of getCloud() bins, with the same numbering,
    and case b's lists get the same hit rows (which equal the model's on that cloud)."""
    m = engine
    c = BC.list_case("b")
    rng = np.random.default_rng(8)
    cells = np.zeros(16 ** 3, np.int8)
    cells[rng.choice(16 ** 3, size=100, replace=False)] = 100
    cells[rng.choice(16 ** 3, size=50, replace=False)] = -1  # (unknown: another class)

    def with_map(env):
        env.setMap([0.0, 0.0, 0.0], [16, 16, 16], cells, 0.5)

    clouds, grids = [], []

    def by_map(env, body, case):
        with_map(env)
        body.fill_map()
        grids.append(body.cells())

    def by_cloud(env, body, case):
        with_map(env)
        clouds.append(env.getCloud())
        body.fill(clouds[-1])
        grids.append(body.cells())

    _, got_map, _, sh_map = run_list_case(m, "b", refill=by_map)
    _, got_cloud, _, sh_cloud = run_list_case(m, "b", refill=by_cloud)
    occupied = int((cells == 100).sum())
    assert sh_map["n"] == sh_cloud["n"] == occupied == len(clouds[0]) and 90 <= occupied <= 100
    assert np.array_equal(grids[0][0], grids[1][0]) and np.array_equal(grids[0][1], grids[1][1])
    assert sh_map["cells"].tolist() == sh_cloud["cells"].tolist() and sh_map["edge"] == sh_cloud["edge"]
    for a, b in zip(got_map[:4], got_cloud[:4]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    assert got_map[4] == got_cloud[4]
    S, n = c["S"], c["n"]
    want_cost, want_hit, want_nb, looked = BM.check(c["sh"], clouds[0], c["count"][:n], c["action"][:n * S], c["cost"][:n * S], S,
                                                    c["parent_id"], c["pst"], c["U"], c["dim"], c["K"], BC.DT, c["n_samp"])
    print("map cloud: %d points, %d of %d looked-at entries blocked" % (occupied, want_nb, looked.sum()))
    assert np.array_equal(got_map[0][:n * S], want_hit) and got_map[4] == 5 + want_nb and 0 < want_nb < looked.sum()


# --------------------------------------------------------------------------------------------------------- poly check
def poly_want(poly, sh, cloud, dim, step):
    """The model on PolyTrajSet.sample (Command form) at the stated times."""
    inf = poly.info()
    K = poly.n
    times = [BM.poly_times(step, inf["total_time"][k]) if inf["status"][k] == 0 and inf["n_segs"][k] > 0 else [0.0] for k in range(K)]
    tt = np.zeros((K, max(len(t) for t in times)))
    for k, t in enumerate(times):
        tt[k, :len(t)] = t
    smp = poly.sample(times=tt)["samples"]
    want = np.full(K, -1, np.int64)
    for k, t in enumerate(times):
        if inf["status"][k] == 0 and inf["n_segs"][k] > 0:
            want[k] = BM.check_poly(sh, cloud, dim, smp[:dim, k, :len(t)].T, smp[2 * dim:3 * dim, k, :len(t)].T)
    return want, inf, [len(t) for t in times]


@pytest.mark.parametrize("dim,K", [(3, 1), (3, 67), (2, 300)], ids=["3d-K1", "3d-K67", "2d-K300"])
def test_poly_check_equals_the_model(engine, dim, K):
    m = engine
    rng = np.random.default_rng(40 + K)
    env = free_env(m, dim, m.ACC, m.workloads.grid_controls([-1.0, 0.0, 1.0], dim))
    w = 5
    wp = rng.uniform(1.0, 7.0, size=(dim, w, K))
    n_wp = rng.integers(2, w + 1, size=K).astype(np.int32)
    if K > 10:
        n_wp[[2, 9]] = 1  # SOLVE_EMPTY: excluded by their status
    r, h = (0.5, 0.25) if dim == 3 else (0.25, 0.125)
    n_pts = 60 if dim == 3 else 10  # (about half of the trajectories meet a point)
    cloud = rng.uniform(0.5, 7.5, size=(n_pts, dim))
    cloud[3, 0] = np.nan
    mct = 0.98 if K == 67 else 0.0  # (K = 67: a tilt limit of 11 degrees, for attitude keys among the hits)
    body = make_body(env, r, h, BC.G, mct)
    body.fill(cloud)
    sh = BM.shape(r, h, BC.G, mct)
    solved = env.solve_traj(wp, n_wp=n_wp, v=1.5)
    total = solved.info()["total_time"]
    loaded = env.load_traj(solved.segments(), solved.dts(), n_segs=np.maximum(n_wp - 1, 0).astype(np.int32))
    k0 = 0 if K == 1 else 5
    steps = (0.25, float(total[k0]) / 8.0)  # (the second: total_k0 is an exact multiple of the step)
    assert np.float64(8) * np.float64(steps[1]) == total[k0]
    seen = set()
    for what, poly in (("solved", solved), ("loaded", loaded), ("scaled", solved)):
        if what == "scaled":
            rows = poly.scale(1.0, 2.0)  # a Lambda on every problem that has segments
            assert (rows["status"][n_wp > 1] == 0).all()
        for step in steps:
            want, inf, counts = poly_want(poly, sh, cloud, dim, step)
            got = body.check_poly(poly, step)
            low = want[want >= 0] & 0xffffffff
            seen |= {"attitude" if x == BM.BAD_ATTITUDE else "point" for x in low} | ({"none"} if (want == -1).any() else set())
            print("%s K %d step %.4f: %d hits (%d attitude), samples %d .. %d" % (
                what, K, step, (want >= 0).sum(), (low == BM.BAD_ATTITUDE).sum(), min(counts), max(counts)))
            assert np.array_equal(got["hit"], want), np.nonzero(got["hit"] != want)[0][:8]
            assert np.array_equal(got["status"], inf["status"]) and got["n_hit"] == (want != -1).sum()
            if K > 10:
                assert got["status"][2] != 0 and got["hit"][2] == -1
        if what == "scaled":
            assert poly.info()["total_time"][k0] != total[k0]  # the Lambda is honoured: the samples run to the scaled total
    if K > 10:
        assert {"point", "none"} <= seen, seen
        # the resident form: the same rows, n_hit added to
        d_hit, d_st, d_n = upload(env, m, np.full(K, PAT64, np.int64)), upload(env, m, np.zeros(K, np.uint8)), upload(env, m, np.array([3], np.int64))
        want, inf, _ = poly_want(loaded, sh, cloud, dim, 0.25)
        body.check_poly_resident(loaded, 0.25, hit=d_hit, status=d_st, n_hit=d_n)
        env.synchronize()
        assert np.array_equal(d_hit.download(np.int64, (K,)), want) and int(d_n.download(np.int64, (1,))[0]) == 3 + (want != -1).sum()
        for b in (d_hit, d_st, d_n):
            b.free()
    for b in (solved, loaded, body):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------------------ the slit
def chain_as_set(m, env, sc, start, actions):
    """The chain's own primitives as a loaded set: c(3) = the control, c(4) = v, c(5) = p of every chain state."""
    info = env.traj_info(start, np.asarray(actions, np.int32).reshape(-1, 1), want_states=True)
    st = info["seg_state"][:, :, 0]
    H = len(actions)
    coeff = np.zeros((H, 4, 6, 1))
    for s in range(H):
        coeff[s, :3, 3, 0], coeff[s, :3, 4, 0], coeff[s, :3, 5, 0] = sc["U"][actions[s]], st[3:6, s], st[0:3, s]
    return env.load_traj(coeff, np.full((H, 1), sc["dt"]), control=m.ACC)


def slit_search(m, env, sc, body, **kw):
    return env.search(sc["start"], sc["goal"], capacity=1 << 14, max_frontier=BC.CAP, sight=False, tol_pos=sc["tol_pos"],
                      body=body, body_samples=BC.N_SAMP, **kw)


def test_the_slit(engine, oracle_lib):
    """tests/body_cases.py: the flat disc rolls through a slit narrower than its diameter, the sphere of the same radius
    does not.  The model's numbers (tests/test_body_model.py runs them on the CPU): FOUND at cost 114.0 in 38 rounds and
    430 expansions along +x, then a_y = +10, 0, -10, +10, 0, -10 at v_x = 2; the sphere runs EMPTY after 47 rounds and 472
    expansions."""
    m = engine
    sc = BC.slit(m)
    want = BC.slit_model_search(m, oracle_lib, sc, BC.FLAT)
    assert (want["out"]["status"], want["cost"], want["out"]["rounds"], want["out"]["expanded"], want["actions"]) == BC.SLIT_FLAT_MODEL
    env = BC.slit_env(m, sc)
    flat = env.alloc_body(*BC.FLAT)
    flat.fill(sc["cloud"])
    res = slit_search(m, env, sc, flat)
    print(res, res.path()[1].tolist() if res.found else None)
    assert res.status == m.search.FOUND and (res.cost, res.rounds, res.expanded) == BC.SLIT_FLAT_MODEL[1:4]
    start, act = res.path()
    assert act.tolist() == BC.SLIT_FLAT_MODEL[4] and res.table.stats() == (want["table"].n_nodes, 0)
    # the path, loaded as a set, is clear of the cloud at the samples of the search; the same path for the sphere is not
    poly = chain_as_set(m, env, sc, start, act.tolist())
    clear = flat.check_poly(poly, sc["dt"] / BC.N_SAMP)
    assert clear["hit"].tolist() == [-1] and clear["n_hit"] == 0
    ball = env.alloc_body(*BC.BALL)
    d_cloud = upload(env, m, sc["cloud"])
    ball.fill_resident(d_cloud, len(sc["cloud"]))
    hit = ball.check_poly(poly, sc["dt"] / BC.N_SAMP)
    assert hit["hit"][0] >= 0 and hit["point"][0] != BM.BAD_ATTITUDE
    p = sc["cloud"][hit["point"][0]]
    assert p[0] == sc["wall_x"] and abs(abs(p[1] - 1.0) - BC.W) < 1e-12  # an edge of the slit
    # the sphere finds no way
    none = slit_search(m, env, sc, ball)
    print(none)
    assert none.status == m.search.EMPTY and not none.found and (none.rounds, none.expanded) == BC.SLIT_BALL_MODEL
    # refused: replanning a body search
    for call in (res.replan, res.replan_timed):
        with pytest.raises(RuntimeError, match="body"):
            call()
    with pytest.raises(RuntimeError, match="body"):
        m.search.replan_prioritised(env, {"results": [res]}, 0.0, 0.25)
    with pytest.raises(RuntimeError, match="body"):
        m.search.refine_prioritised(env, {"results": [res]}, 0.25)
    with pytest.raises(ValueError, match="body"):
        m.search.plan_prioritised(env, sc["start"].reshape(-1, 1), sc["goal"].reshape(1, -1), 0.25, 0.3, body=flat)
    for b in (poly, res, none, flat, ball, d_cloud):
        b.free()
    env.close()


def test_improve_goes_on_with_the_body(engine):
    """A greedy body search (eps = 3), then improve(1.0): the optimum of the plain body search, through the slit; a cloud
    filled again in between is an error."""
    m = engine
    sc = BC.slit(m)
    env = BC.slit_env(m, sc)
    flat = env.alloc_body(*BC.FLAT)
    flat.fill(sc["cloud"])
    first = slit_search(m, env, sc, flat, eps=3.0)
    assert first.found and first.cost >= BC.SLIT_FLAT_MODEL[1]
    e0 = first.expanded
    best = first.improve(1.0)
    print(first.cost, "->", best.cost, "expanded", e0, "->", best.expanded)
    assert best.found and best.cost == BC.SLIT_FLAT_MODEL[1] and best.expanded >= e0
    start, act = best.path()
    poly = chain_as_set(m, env, sc, start, act.tolist())
    assert flat.check_poly(poly, sc["dt"] / BC.N_SAMP)["hit"].tolist() == [-1]
    staged, stages = env.anytime(best, [1.0, 0.5])
    assert staged.found and staged.cost == best.cost and len(stages) >= 1
    flat.fill(sc["cloud"])
    with pytest.raises(RuntimeError, match="generation"):
        staged.improve(0.5)
    for b in (poly, staged, flat):
        b.free()
    env.close()


# ----------------------------------------------------------------------------------------- nothing changes without it
def test_an_empty_cloud_changes_nothing(engine):
    """search and search_many with body=None against the same calls with a body over an empty cloud (the corridor's
    controls of 0.5 m/s^2 never fail the attitude test): the same tables, byte for byte."""
    m = engine
    env, start, goal = corridor_env(m)
    starts, goals = corridor_queries(m)
    body = env.alloc_body(0.3, 0.1)
    body.fill(np.zeros((0, 2)))
    assert body.shape()["n"] == 0 and body.shape()["cells"].tolist() == [1, 1, 1]
    kw = dict(capacity=1 << 15, max_frontier=4096)
    a, b = env.search(start, goal, **kw), env.search(start, goal, body=body, body_samples=3, **kw)
    ma, mb = env.search_many(starts, goals, **kw), env.search_many(starts, goals, body=body, **kw)
    assert (a.status, a.cost, a.rounds, a.expanded) == (b.status, b.cost, b.rounds, b.expanded) and a.cost == 351.5
    assert (ma.status, ma.cost, ma.rounds, ma.expanded, ma.total_rounds) == (mb.status, mb.cost, mb.rounds, mb.expanded, mb.total_rounds)
    for x, y in ((a, b), (ma, mb)):
        tx, ty = x.table.download(), y.table.download()
        assert tx.keys() == ty.keys() and tx["n_nodes"] == ty["n_nodes"] > 1000
        for key in tx:
            assert np.array_equal(np.atleast_1d(tx[key]).view(np.uint8), np.atleast_1d(ty[key]).view(np.uint8)), key
    assert np.array_equal(a.path()[1], b.path()[1])
    assert b._params["body"] is body and b._params["body_generation"] == body.generation and a._params.get("body") is None
    for x in (a, b, ma, mb, body):
        x.free()
    env.close()


# ------------------------------------------------------------------------------------------------- errors and no-ops
def test_errors_and_no_ops(engine):
    m = engine
    A = m._abi
    L_ = A.lib()
    env, start, goal = corridor_env(m)
    F = env.n_fields

    def code(fn):
        with pytest.raises(A.MplxError) as e:
            fn()
        return e.value.code

    raw = lambda rc: A.check(env._ctx, rc)
    body = env.alloc_body(0.3, 0.1)
    for r, h, g, mct in ((0.0, 0.1, 9.81, 0.0), (np.nan, 0.1, 9.81, 0.0), (np.inf, 0.1, 9.81, 0.0), (0.3, -1.0, 9.81, 0.0),
                         (0.3, 0.1, 0.0, 0.0), (0.3, 0.1, np.inf, 0.0), (0.3, 0.1, 9.81, 1.0), (0.3, 0.1, 9.81, -0.1),
                         (0.3, 0.1, 9.81, np.nan), (1e200, 0.1, 9.81, 0.0)):
        assert code(lambda: body.set_shape(r, h, g, min_cos_tilt=mct)) == A.ERR_ARG, (r, h, g, mct)
    assert body.min_cos_tilt == 0.0 and env.alloc_body(0.3, 0.1, tilt_max=math.pi / 3).min_cos_tilt == math.cos(math.pi / 3)
    Ls = m.Lists(env, 4, 9, want_state=False, stride=9)
    Ls.count.upload(np.array([1, 0, 0, 0], np.int32))
    Ls.action.upload(np.zeros(36, np.int32))
    Ls.cost.upload(np.ones(36))
    fr = m.TableFrontier(env, 4)
    fr.id.upload(np.zeros(4, np.int32))
    fr.state.upload(np.zeros((F, 4)))
    assert code(lambda: body.check(fr, Ls, 4)) == A.ERR_STATE                      # no cloud yet
    assert code(lambda: body.cells()) == A.ERR_STATE
    with pytest.raises(ValueError, match="cloud"):
        env.search(start, goal, body=body)
    # the fills
    one = np.zeros((1, 2))
    assert code(lambda: raw(L_.mplx_body_fill(body._body, one.ctypes.data, -1))) == A.ERR_ARG
    assert code(lambda: raw(L_.mplx_body_fill(body._body, None, 3))) == A.ERR_ARG
    assert code(lambda: raw(L_.mplx_body_fill(body._body, one.ctypes.data, 1 << 31))) == A.ERR_ARG        # n > 2^31 - 2
    assert code(lambda: raw(L_.mplx_body_fill_device(body._body, fr.ptr, (1 << 26) + 1))) == A.ERR_ARG    # over 1 GiB in 2-D
    assert code(lambda: raw(L_.mplx_body_fill_device(body._body, None, 3))) == A.ERR_ARG
    assert code(lambda: body.fill_map(7)) == A.ERR_ARG
    bare = m.EnvMap(2)
    nomap = bare.alloc_body(0.3, 0.1)
    assert code(lambda: nomap.fill_map()) == A.ERR_STATE                           # no map
    nomap.fill(one)
    Lb = m.Lists(bare, 4, 9, want_state=False, stride=9)
    frb = m.TableFrontier(bare, 4)
    assert code(lambda: nomap.check(frb, Lb, 4)) == A.ERR_STATE                    # no params, no controls
    # before a shape
    fresh = C.c_void_p()
    raw(L_.mplx_body_create(env._ctx, C.byref(fresh)))
    raw(L_.mplx_body_fill(fresh, one.ctypes.data, 1))
    s = Ls.c_struct()
    assert code(lambda: raw(L_.mplx_body_check_device(fresh, C.byref(s), 4, fr.id.ptr, fr.ptr, 4, 4, None, None))) == A.ERR_STATE
    L_.mplx_body_destroy(fresh)
    assert L_.mplx_body_create(env._ctx, None) == A.ERR_ARG and L_.mplx_body_create(None, C.byref(fresh)) == A.ERR_ARG
    # the list check
    body.fill(np.array([[50.0, 50.0]]))
    for n_samp in (0, -3):
        assert code(lambda: body.check(fr, Ls, 4, n_samp)) == A.ERR_ARG
    assert code(lambda: body.check(fr, Ls, -1)) == A.ERR_ARG
    assert code(lambda: body.check(fr, Ls, 5)) == A.ERR_ARG                        # parent_stride < n_nodes
    no_cost = Ls.c_struct()
    no_cost.cost = None
    assert code(lambda: raw(L_.mplx_body_check_device(body._body, C.byref(no_cost), 4, fr.id.ptr, fr.ptr, 4, 4, None, None))) == A.ERR_ARG
    assert code(lambda: raw(L_.mplx_body_check_device(body._body, None, 4, fr.id.ptr, fr.ptr, 4, 4, None, None))) == A.ERR_ARG
    assert code(lambda: raw(L_.mplx_body_check_device(body._body, C.byref(s), 4, None, fr.ptr, 4, 4, None, None))) == A.ERR_ARG
    assert code(lambda: raw(L_.mplx_body_check_device(body._body, C.byref(s), 4, fr.id.ptr, None, 4, 4, None, None))) == A.ERR_ARG
    assert L_.mplx_body_check_device(None, C.byref(s), 4, fr.id.ptr, fr.ptr, 4, 4, None, None) == A.ERR_ARG
    # no-ops: no rows; a cloud that is far away; an empty cloud
    d_hit = upload(env, m, np.full(36, 7, np.int64))
    body.check(fr, Ls, 0, hit=d_hit)
    env.synchronize()
    assert np.all(d_hit.download(np.int64, (36,)) == 7)
    for pts in (np.array([[50.0, 50.0]]), np.zeros((0, 2)), np.array([[np.nan, 0.0], [0.0, np.inf]])):
        body.fill(pts)
        body.check(fr, Ls, 4, hit=d_hit)
        env.synchronize()
        assert np.all(d_hit.download(np.int64, (36,)) == -1) and np.all(Ls.cost.download(np.float64, (36,)) == 1.0)
    assert body.shape()["n_excluded"] == 2
    body.fill(np.zeros((1, 2)))  # the parent sits on it
    body.check(fr, Ls, 4, hit=d_hit)
    env.synchronize()
    assert d_hit.download(np.int64, (36,)).tolist() == [0] + [-1] * 35 and Ls.cost.download(np.float64, (36,))[0] == np.inf
    # the set check
    wp = np.array([[[1.0], [2.0], [3.0]], [[1.0], [1.5], [1.0]]])
    poly = env.solve_traj(wp, v=1.0)
    i, o = A.BodyPolyIn(), A.BodyPolyOut()
    for step in (0.0, -1.0, np.inf, np.nan):
        assert code(lambda: body.check_poly(poly, step)) == A.ERR_ARG, step
    i.step = 0.25
    assert code(lambda: raw(L_.mplx_body_check_poly(body._body, None, C.byref(i), C.byref(o)))) == A.ERR_ARG
    assert code(lambda: raw(L_.mplx_body_check_poly(body._body, poly._h, None, C.byref(o)))) == A.ERR_ARG
    assert code(lambda: raw(L_.mplx_body_check_poly_device(body._body, poly._h, C.byref(i), None))) == A.ERR_ARG
    env2, _, _ = corridor_env(m)
    other = env2.solve_traj(wp, v=1.0)
    assert code(lambda: raw(L_.mplx_body_check_poly(body._body, other._h, C.byref(i), C.byref(o)))) == A.ERR_ARG   # another context
    unsolved = env.alloc_poly(4, 3)
    assert code(lambda: raw(L_.mplx_body_check_poly(body._body, unsolved._h, C.byref(i), C.byref(o)))) == A.ERR_STATE
    unfilled = env.alloc_body(0.3, 0.1)
    assert code(lambda: raw(L_.mplx_body_check_poly(unfilled._body, poly._h, C.byref(i), C.byref(o)))) == A.ERR_STATE
    raw(L_.mplx_body_check_poly(body._body, poly._h, C.byref(i), C.byref(o)))      # every output optional
    # the Python layer
    with pytest.raises(TypeError):
        env.search(start, goal, body="a body")
    with pytest.raises(ValueError, match="body_samples"):
        env.search(start, goal, body=body, body_samples=0)
    for b in (d_hit, poly, other, unsolved, unfilled, nomap, Lb, frb, fr, Ls, body):
        b.free()
    bare.close()
    env2.close()
    env.close()
