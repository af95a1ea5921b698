"""MapUtil<Dim>::rayTrace and the ray trace of env_map::is_goal on the device (include/mplx_ray.h, csrc/ray_kernel.hip)
against the numpy restatement (tests/ray_model.py, pinned on the CPU to the reference's own MapUtil and env_map by
tests/test_ray.py) and the committed fixture: every output row bit for bit, cell order included, under every lanes-
per-ray instantiation; round boundaries, wave tails, cell_cap, BAD rays, x lengths, the map as edited on the device,
a full-size run, the goal pass on the lists of every route, argument and state errors."""
import ctypes as C
import os

import numpy as np
import pytest

import ray_model as R
from test_ray import GOLDEN, fixture_model

LANES = [0, 4, 16, 64]
POISON = -0x5A5A5A5B


def device_trace(env, p1, p2, cell_cap=0, lanes=0, n=None, want_counts=True):
    """mplx_ray_trace_device on uploaded points ([n][D] rows; p2 one point [D]: the broadcast form); cells start
    poisoned."""
    p1 = np.asarray(p1, dtype=np.float64)
    n_all = len(p1)
    n = n_all if n is None else n
    d1 = engine_array(env, np.ascontiguousarray(p1.T))
    p2 = np.asarray(p2, dtype=np.float64)
    one = p2.ndim == 1
    d2 = engine_array(env, p2 if one else np.ascontiguousarray(p2.T))
    out = env.alloc_rays(n, cell_cap, want_counts)
    if cell_cap:
        out.cells.upload(np.full((n, cell_cap), POISON, np.int32))
    env.ray_trace_resident(d1, d2, out, n=n, stride=n_all, p2_stride=0 if one else n_all, lanes=lanes)
    env.synchronize()
    got = out.download()
    for b in (d1, d2, out):
        b.free()
    return got


def engine_array(env, host):
    from motion_primitive_library_amd.env import DeviceArray
    host = np.ascontiguousarray(host)
    buf = DeviceArray(env, max(host.nbytes, 8))
    buf.upload(host)
    return buf


def assert_rays(got, m, cap=0, what="", n=None):
    n = m["n_cells"].size if n is None else n
    want_cells, want_status = R.cells_matrix(m, cap, POISON) if cap else (None, m["status"])
    for k, want in (("status", want_status), ("n_cells", m["n_cells"]), ("first_hit", m["first_hit"])):
        if k in got:
            bad = np.nonzero(got[k] != want[:n])[0]
            assert bad.size == 0, "%s: %s differs for %d rays, first %s got %s want %s" % (what, k, bad.size, bad[:5], got[k][bad[:5]], want[:n][bad[:5]])
    if cap:
        bad = np.argwhere(got["cells"] != want_cells[:n])
        assert bad.shape[0] == 0, "%s: cells differ in %d entries, first (ray, slot) %s" % (what, bad.shape[0], bad[:3].tolist())


def make_env(engine, case):
    name, dim, grid, md, org, res = case
    env = engine.EnvMap(dim)
    env.setMap(org, md, grid, res)
    return env


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.fixture_cases(), ids=[c[0] for c in R.fixture_cases()])
def test_device_rays_equal_model_and_fixture(engine, case):
    """Device call == model == fixture for lanes 0, 4, 16, 64; the host-pointer call and the broadcast p2 give the
    same."""
    name, dim, grid, md, org, res = case
    z = np.load(GOLDEN)
    p1, p2, m = fixture_model(case)
    assert np.array_equal(m["n_cells"], z[name + "/n_cells"]) and np.array_equal(m["first_hit"], z[name + "/first_hit"])
    assert np.array_equal(m["cells"], np.cumsum(z[name + "/cell_steps"].astype(np.int64)).astype(np.int32))
    cap = int(m["n_cells"].max())
    env = make_env(engine, case)
    for lanes in LANES:
        got = device_trace(env, p1, p2, cap, lanes)
        assert_rays(got, m, cap, "%s lanes %d" % (name, lanes))
        goal, _ = R.is_goal(m, p1, p2, R.TOL_POS)
        inside = np.abs(p1 - p2).max(axis=1) <= R.TOL_POS
        assert np.array_equal(inside & ((got["status"] & R.HIT) == 0), z[name + "/is_goal"] != 0)
    # host pointers
    cells = np.full((len(p1), cap), POISON, np.int32)
    host = env.ray_trace(p1.T, p2.T, cell_cap=cap, cells=cells)
    assert_rays(host, m, cap, name + " host pointers")
    counts = env.ray_trace(p1.T, p2.T)
    assert "cells" not in counts
    assert_rays(counts, m, 0, name + " host pointers, counts only")
    # one p2 for all rays == the expanded array
    goal_pt = p2[5].copy()
    mb = R.ray_trace(grid, md, org, res, p1, np.broadcast_to(goal_pt, p1.shape))
    capb = int(mb["n_cells"].max())
    for lanes in (0, 4):
        assert_rays(device_trace(env, p1, goal_pt, capb, lanes), mb, capb, name + " broadcast p2")
        assert_rays(device_trace(env, p1, np.broadcast_to(goal_pt, p1.shape).copy(), capb, lanes), mb, capb, name + " expanded p2")
    cells = np.full((len(p1), capb), POISON, np.int32)
    assert_rays(env.ray_trace(p1.T, goal_pt, cell_cap=capb, cells=cells), mb, capb, name + " broadcast p2, host pointers")
    env.close()


@pytest.mark.gpu
def test_round_boundaries_wave_tails_and_cell_cap(engine):
    p1, p2, classes = R.boundary_set()
    grid = R.boundary_map()
    case = ("boundary", 2, grid, R.BOUNDARY_MD, R.BOUNDARY_ORG, R.BOUNDARY_RES)
    m = R.ray_trace(grid, R.BOUNDARY_MD, R.BOUNDARY_ORG, R.BOUNDARY_RES, p1, p2)
    longest = int(m["n_cells"].max())
    assert longest >= 100 and len(p1) >= 33
    env = make_env(engine, case)
    for lanes in LANES:
        assert_rays(device_trace(env, p1, p2, longest, lanes), m, longest, "boundary set, lanes %d" % lanes)
    # wave tails: the last wave holds 1, 64/G - 1, 64/G, 64/G + 1 rays; 257 rays
    big1, big2 = np.tile(p1, (9, 1))[:257], np.tile(p2, (9, 1))[:257]
    mb = R.ray_trace(grid, R.BOUNDARY_MD, R.BOUNDARY_ORG, R.BOUNDARY_RES, big1, big2)
    for lanes in (4, 16, 64):
        per_wave = 64 // lanes
        for n in sorted({1, per_wave - 1, per_wave, per_wave + 1, 257} - {0}):
            got = device_trace(env, big1, big2, longest, lanes, n=n)
            assert got["status"].shape == (n,)
            assert_rays(got, mb, longest, "wave tail n %d, lanes %d" % (n, lanes), n=n)
    # cell_cap in {1, n - 1, n, n + 1} on a poisoned buffer: prefix, untouched tail, TRUNCATED exactly when due
    for cap in (1, longest - 1, longest, longest + 1):
        for lanes in LANES:
            got = device_trace(env, p1, p2, cap, lanes)
            assert_rays(got, m, cap, "cell_cap %d, lanes %d" % (cap, lanes))
            assert np.array_equal((got["status"] & R.TRUNCATED) > 0, m["n_cells"] > cap)
            assert ((got["cells"] == POISON).sum(axis=1) == cap - np.minimum(m["n_cells"], cap)).all()
    assert ((device_trace(env, p1, p2, longest - 1, 0)["status"] & R.TRUNCATED) > 0).sum() >= 1
    # cells == NULL: counts only, never TRUNCATED; status alone
    got = device_trace(env, p1, p2, 0, 16)
    assert_rays(got, m, 0, "no cells")
    got = device_trace(env, p1, p2, 0, 4, want_counts=False)
    assert set(got) == {"status"} and np.array_equal(got["status"], m["status"])
    env.close()


@pytest.mark.gpu
def test_bad_rays_between_good_ones(engine):
    case = R.fixture_cases()[1]
    name, dim, grid, md, org, res = case
    p1, p2, _ = fixture_model(case)
    p1, p2 = p1[:300].copy(), p2[:300].copy()
    bad = [3, 64, 65, 127, 200, 299]
    p1[3, 0] = np.nan
    p2[64, 1] = np.inf
    p1[65, 2] = -np.inf
    p2[127, 0] = 1e300
    p1[200] = 1e300
    p2[200] = -1e300
    p1[299, 1], p2[299, 1] = 1.7e308, -1.7e308  # the difference overflows
    m = R.ray_trace(grid, md, org, res, p1, p2)
    assert ((m["status"] & R.BAD) > 0).nonzero()[0].tolist() == bad and (m["n_cells"][bad] == 0).all()
    cap = int(m["n_cells"].max())
    env = make_env(engine, case)
    for lanes in LANES:
        got = device_trace(env, p1, p2, cap, lanes)
        assert_rays(got, m, cap, "BAD rays, lanes %d" % lanes)
        assert (got["status"][bad] == R.BAD).all() and (got["n_cells"][bad] == 0).all() and (got["first_hit"][bad] == -1).all()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_maps_with_short_and_unaligned_rows(engine, dim):
    """x lengths 1, 15, 17, 33 with unequal other axes: row ends and unaligned bytes."""
    from test_map_util import x_case
    for d0 in (1, 15, 17, 33):
        case = x_case(d0, dim)
        name, _, grid, md, org, res = case
        assert len(set(md)) == len(md)
        p1, p2 = R.fixture_rays(case, n=700)
        rng = np.random.default_rng(d0)  # a third of the rays with both ends inside the map, however narrow it is
        p1[::3] = np.asarray(org) + rng.uniform(0, 1, size=p1[::3].shape) * np.asarray(md) * res
        p2[::3] = np.asarray(org) + rng.uniform(0, 1, size=p2[::3].shape) * np.asarray(md) * res
        m = R.ray_trace(grid, md, org, res, p1, p2)
        assert m["n_cells"].max() >= 3 and ((m["status"] & R.HIT) > 0).sum() >= 5 and ((m["status"] & R.LEFT_MAP) > 0).sum() >= 5
        cap = int(m["n_cells"].max())
        env = make_env(engine, case)
        for lanes in LANES:
            assert_rays(device_trace(env, p1, p2, cap, lanes), m, cap, "%s lanes %d" % (name, lanes))
        env.close()


@pytest.mark.gpu
def test_rays_follow_the_device_map(engine):
    """After editMap, dilate and updatePotentialMap the rays see the resulting cells, and no ray call uploads a map."""
    from test_map_util import box, np_dilate
    case = R.fixture_cases()[0]
    name, dim, grid, md, org, res = case
    p1, p2, m0 = fixture_model(case)
    p1, p2 = p1[:1500], p2[:1500]
    env = make_env(engine, case)
    up0 = env.map_upload_bytes()
    cap = int(m0["n_cells"].max())
    # editMap: free every cell that was a first hit, occupy the last cell of some clear rays
    cur = np.array(grid, dtype=np.int8)
    hits = np.unique(m0["first_hit"][:1500][m0["first_hit"][:1500] >= 0])[::2]
    clear = np.nonzero((m0["first_hit"][:1500] < 0) & (m0["n_cells"][:1500] > 0))[0][::3]
    occupy = np.unique(m0["cells"][m0["offs"][clear + 1] - 1])
    idx = np.concatenate([hits, occupy])
    val = np.concatenate([np.zeros(hits.size, np.int8), np.full(occupy.size, 100, np.int8)])
    env.editMap(idx, val)
    up1 = env.map_upload_bytes()
    assert up1 - up0 <= idx.size * 16
    cur[idx] = val
    m = R.ray_trace(cur, md, org, res, p1, p2)
    assert (m["first_hit"] != m0["first_hit"][:1500]).sum() > 50
    assert_rays(device_trace(env, p1, p2, cap), m, cap, "after editMap")
    assert env.map_upload_bytes() == up1
    cur = np_dilate(cur, md, box(dim))
    assert np.array_equal(env.dilate(box(dim)), cur)
    m = R.ray_trace(cur, md, org, res, p1, p2)
    up2 = env.map_upload_bytes()
    assert_rays(device_trace(env, p1, p2, cap, 16), m, cap, "after dilate")
    assert env.map_upload_bytes() == up2
    centre = [float(org[i] + md[i] * res / 2) for i in range(dim)]
    cur = env.updatePotentialMap(centre, [0.4] * dim)
    assert ((cur > 0) & (cur < 100)).sum() > 100
    up3 = env.map_upload_bytes()
    m = R.ray_trace(cur, md, org, res, p1, p2)
    assert_rays(device_trace(env, p1, p2, cap, 4), m, cap, "after updatePotentialMap")
    host = env.ray_trace(p1.T, p2.T)
    assert_rays(host, m, 0, "after updatePotentialMap, host pointers")
    assert env.map_upload_bytes() == up3
    env.close()


@pytest.mark.gpu
def test_rays_across_a_256_cube(engine):
    W = engine.workloads
    md, org, res = [256] * 3, [0.0] * 3, 0.1
    grid = W.box_map(md, res, 0.1, 2056).ravel()
    rng = np.random.default_rng(2057)
    n = 16384
    p1 = rng.uniform(0.0, 25.6, size=(n, 3))
    p2 = rng.uniform(0.0, 25.6, size=(n, 3))
    m = R.ray_trace(grid, md, org, res, p1, p2)
    assert m["n_cells"].max() > 250 and 0.2 < ((m["status"] & R.HIT) > 0).mean() < 0.98
    cap = int(m["n_cells"].max())
    env = make_env(engine, ("cube", 3, grid, md, org, res))
    assert_rays(device_trace(env, p1, p2, cap, 0), m, cap, "256^3")
    for lanes in (4, 16):
        assert_rays(device_trace(env, p1[:2048], p2[:2048], 0, lanes), m, 0, "256^3 lanes %d" % lanes, n=2048)
    env.close()


class _At:
    """A device pointer `off` bytes into a DeviceArray."""

    def __init__(self, buf, off):
        self.ptr = buf.ptr + off


def _emitted(L):
    S = L["stride"]
    return np.nonzero((np.arange(S)[None, :] < L["count"][:, None]).ravel())[0]


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_goal_pass_on_the_goal_world(engine, dim):
    from helpers import engine_env
    wl, goal, tol = R.goal_world(engine, dim)
    blocked_seen = clear_seen = 0
    reference = None
    for route in ("grid", "tile", "dense", "post", "post+goal_or_null", "post+unaligned"):
        env = engine_env(engine, wl)
        if not route.startswith("post"):
            env.set_lists_route(route)
        fr = env.upload_frontier(wl.nodes)
        env.set_goal(goal, w=10.0, v_max=2.0, tol_pos=tol)
        lists = env.alloc_lists(wl.n_nodes, want_state=True, want_flags=True)
        # non-emitted slots start with bit 0 set: the pass must not take them for candidates
        lists.flags.upload(np.full(lists.n_slots, 0xA5, np.uint8))
        env.expand_lists_resident(fr, lists)
        env.synchronize()
        L = lists.download()
        emit = _emitted(L)
        flags_dev = None
        if route.startswith("post"):
            post = env.post_lists(lists, goal, w=10.0, v_max=2.0, tol_pos=tol)["flags"]
            assert np.array_equal(post[emit] & 3, L["flags"][emit] & 3)
            post[np.setdiff1d(np.arange(post.size), emit)] = 0xA5
            # (unaligned: the row starts 3 bytes into an allocation -- 13 bytes before the first 16-byte boundary of
            # the scan, 3 after its last full vector)
            off = 3 if route == "post+unaligned" else 0
            padded = np.concatenate([np.full(off, 0xA5, np.uint8), post, np.full(32 - off, 0xA5, np.uint8)])
            flags_buf = engine_array(env, padded)
            flags_dev = _At(flags_buf, off)
            before = post.copy()
        else:
            assert env.last_lists_route() == route
            before = L["flags"].copy()
        in_tol, blocked = R.goal_world_model(wl, goal, tol, L["state"][:dim, emit])
        assert np.array_equal((before[emit] & 1) > 0, in_tol)
        if route == "post+goal_or_null":
            env.set_goal(None)
            env.goal_sight(lists, flags=flags_dev, goal_row=goal, tol_pos=tol)
        else:
            env.goal_sight(lists, flags=flags_dev)
        env.synchronize()
        if flags_dev:
            whole = flags_buf.download(np.uint8, (padded.size,))
            after = whole[off:off + lists.n_slots]
            assert (whole[:off] == 0xA5).all() and (whole[off + lists.n_slots:] == 0xA5).all()
        else:
            after = lists.flags.download(np.uint8, (lists.n_slots,))
        assert np.array_equal((after[emit] & 8) > 0, blocked), route
        assert np.array_equal((after[emit] & 9) == 1, in_tol & ~blocked), route
        want = before.copy()
        want[emit[blocked]] |= 8
        bad = np.nonzero(after != want)[0]
        assert bad.size == 0, "%s: %d flag bytes changed that must not, first %s" % (route, bad.size, bad[:5])
        blocked_seen, clear_seen = int(blocked.sum()), int((in_tol & ~blocked).sum())
        assert blocked_seen >= 30 and clear_seen >= 30
        if reference is None:
            reference = after[emit] & 9
        assert np.array_equal(after[emit] & 9, reference), route
        # a second pass changes nothing
        if route == "grid":
            env.goal_sight(lists)
            env.synchronize()
            assert np.array_equal(lists.flags.download(np.uint8, (lists.n_slots,)), after)
        for b in (lists, fr) + ((flags_buf,) if flags_dev else ()):
            b.free()
        env.close()


@pytest.mark.gpu
def test_argument_and_state_errors(engine):
    _abi = engine._abi
    L = _abi.lib()
    case = R.fixture_cases()[0]
    name, dim, grid, md, org, res = case
    p1, p2, m = fixture_model(case)
    p1, p2 = p1[:64], p2[:64]
    n = 64
    env = engine.EnvMap(dim)
    d1, d2 = engine_array(env, np.ascontiguousarray(p1.T)), engine_array(env, np.ascontiguousarray(p2.T))
    out = env.alloc_rays(n, 8)

    def call(fn=L.mplx_ray_trace_device, a=None, b=None, count=n, stride=n, p2_stride=n, lanes=0, edit=None, null_out=False):
        o = out.c_struct()
        if edit:
            edit(o)
        return fn(env._ctx, d1.ptr if a is None else a, d2.ptr if b is None else b, count, stride, p2_stride, lanes,
                  None if null_out else C.byref(o))

    assert call() == _abi.ERR_STATE  # no map
    env.setMap(org, md, grid, res)
    assert call() == _abi.OK
    env.synchronize()
    assert np.array_equal(out.download()["n_cells"], m["n_cells"][:n])
    assert call(count=-1) == _abi.ERR_ARG
    assert call(stride=n - 1) == _abi.ERR_ARG
    assert call(null_out=True) == _abi.ERR_ARG
    assert call(edit=lambda o: setattr(o, "status", None)) == _abi.ERR_ARG
    assert call(a=0) == _abi.ERR_ARG and call(b=0) == _abi.ERR_ARG
    for lanes in (1, 5, 8, 32, 128, -4):
        assert call(lanes=lanes) == _abi.ERR_ARG
    assert call(edit=lambda o: setattr(o, "cell_cap", -1)) == _abi.ERR_ARG
    assert call(edit=lambda o: setattr(o, "cell_cap", 0)) == _abi.ERR_ARG  # cells given
    assert call(count=0, a=0, b=0) == _abi.OK
    # the host-pointer call checks the same
    h1, h2 = np.ascontiguousarray(p1.T), np.ascontiguousarray(p2.T)
    st = np.zeros(n, np.uint8)
    o = _abi.RayOut()
    o.status = st.ctypes.data
    assert L.mplx_ray_trace(env._ctx, h1.ctypes.data, h2.ctypes.data, n, n, n, 0, C.byref(o)) == _abi.OK
    assert np.array_equal(st, m["status"][:n])
    assert L.mplx_ray_trace(env._ctx, h1.ctypes.data, h2.ctypes.data, n, n - 1, n, 0, C.byref(o)) == _abi.ERR_ARG
    assert L.mplx_ray_trace(env._ctx, None, h2.ctypes.data, n, n, n, 0, C.byref(o)) == _abi.ERR_ARG
    assert L.mplx_ray_trace(env._ctx, h1.ctypes.data, h2.ctypes.data, n, n, n, 7, C.byref(o)) == _abi.ERR_ARG
    o.status = None
    assert L.mplx_ray_trace(env._ctx, h1.ctypes.data, h2.ctypes.data, n, n, n, 0, C.byref(o)) == _abi.ERR_ARG
    with pytest.raises(_abi.MplxError):
        env.ray_trace(p1.T, p2.T, lanes=3)
    # the goal pass
    env.set_control(0x03)
    env.set_u(engine.workloads.grid_controls([-1.0, 0.0, 1.0], dim))
    env.set_dt(0.5)
    nodes = np.zeros((4 * dim + 2, 4))
    nodes[:dim] = np.asarray(org)[:, None] + 1.0
    fr = env.upload_frontier(nodes)
    lists = env.alloc_lists(4, want_state=True)
    env.expand_lists_resident(fr, lists)
    flags = engine_array(env, np.zeros(lists.n_slots, np.uint8))
    goal = np.ascontiguousarray(nodes[:, 0])

    def sight(s=None, nodes_n=4, fl=flags.ptr, spec=None):
        s = lists.c_struct() if s is None else s
        return L.mplx_goal_sight_device(env._ctx, C.byref(s), nodes_n, spec, fl)

    assert sight() == _abi.ERR_STATE  # no goal from either source
    g = _abi.GoalSpec()
    g.goal, g.control, g.tol_pos = goal.ctypes.data, 0x03, 0.5
    assert sight(spec=C.byref(g)) == _abi.OK
    env.set_goal(goal, tol_pos=0.5)
    assert sight() == _abi.OK
    assert sight(fl=None) == _abi.ERR_ARG
    assert sight(nodes_n=-1) == _abi.ERR_ARG
    assert sight(nodes_n=0) == _abi.OK
    for field in ("count", "state"):
        s = lists.c_struct()
        setattr(s, field, None)
        assert sight(s=s) == _abi.ERR_ARG, field
    env.synchronize()
    env2 = engine.EnvMap(dim)  # no map
    assert L.mplx_goal_sight_device(env2._ctx, C.byref(lists.c_struct()), 4, C.byref(g), flags.ptr) == _abi.ERR_STATE
    env2.close()
    for b in (d1, d2, out, fr, lists, flags):
        b.free()
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.fixture_cases()[:2], ids=["d2", "d3"])
def test_map_util_ray_trace_returns_the_references_cells(engine, case):
    """MapUtil.rayTrace: (n, D) int32 cell coordinates in the reference's order, as vec_Veci; an empty list too."""
    name, dim, grid, md, org, res = case
    p1, p2, m = fixture_model(case)
    mu = engine.MapUtil(dim)
    mu.setMap(org, md, grid, res)
    picks = [int(np.argmax(m["n_cells"])), int(np.argmin(m["n_cells"]))] + list(range(20))
    assert m["n_cells"][picks[1]] == 0
    for k in picks:
        cells = mu.rayTrace(p1[k], p2[k])
        want = m["cells"][m["offs"][k]:m["offs"][k + 1]].astype(np.int64)
        assert cells.dtype == np.int32 and cells.shape == (want.size, dim), (name, k)
        coords = np.stack([want % md[0], want // md[0] % md[1]] + ([want // (md[0] * md[1])] if dim == 3 else []), axis=1)
        assert np.array_equal(cells, coords), (name, k)
    # one ray through EnvMap.ray_trace with single points
    env = make_env(engine, case)
    k = picks[0]
    one = env.ray_trace(p1[k], p2[k], cell_cap=int(m["n_cells"][k]))
    assert one["status"].shape == (1,) and one["n_cells"][0] == m["n_cells"][k]
    assert np.array_equal(one["cells"][0], m["cells"][m["offs"][k]:m["offs"][k + 1]])
    env.close()
