"""Anisotropic, word-unaligned maps through every kernel that turns a cell coordinate into an address.

Every such kernel uses the map's own axis lengths: the flat cell index x + d0 * (y + d1 * z), the blocked-bit map
(packed in flat order, no padding per row), the reach box staged from it into LDS, the summed-area table with its
(d0 + 1)(d1 + 1) strides, the neighbour reads of the potential map's gradient term, the cells the edge re-validation
walks.  On a cube an exchange of d0 and d1 in any one of them goes unnoticed, and so does a row length rounded to a
word when the edge is a multiple of 32 -- and the suite's mid-size maps were cubes with friendly edges.  Here the axes
differ and the x length is not a multiple of 4.

CPU: the restatement against the reference build on these worlds (a); the worlds do discriminate -- enough free and
blocked successors, and an oracle given the same cells with two axis lengths exchanged answers differently (b); a
committed fixture made by the reference build pins the oracle on machines without that build (c).
GPU: every (shape, configuration, route) against the reference (d), the pair kernel against the general one (e), the
edge kernel (f), and map preparation (potential map, search region, dilate, cell edits) feeding the expansion (g).

Kernels observed per configuration (asserted below): VEL / ACC / JRK on occupancy -> route grid, kernel lex; SNP on
occupancy and everything on a potential map -> route grid, kernel grid; yaw controls on a potential map over a
pre-screened frontier -> kernel pair; routes tile and dense run their own kernels (last_grid_kernel() == "none")."""
import hashlib
import os

import numpy as np
import pytest

from helpers import assert_lists_equal, assert_slots_equal, engine_env, odd_world, oracle_env, require_reference_build
from oracle import oracle as O
from test_gpu_parity import YAW_COST_RTOL, _small_world

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry_golden.npz")
N_NODES = 160

SHAPES = [
    [53, 37, 29],  # all odd, pairwise different; n_cells is odd: the last blocked-bit word is partial
    [29, 53, 37],  # the same lengths permuted: the long axis moves
    [80, 17, 33],  # d0 % 32 == 16 and d0 % 16 == 0: the 16-byte vector paths with half-word rows; d1 shorter than a reach box
    [16, 48, 31],  # two x rows per bit word
    [33, 40, 96],  # one cell over a word, long in z
    [75, 43],      # 2D: odd, different, no multiple of 4
    [43, 75],      # ... permuted
    [33, 96],      # one cell over a word, long in y
]

# (name, control, potential map, gradient weight, search region, heading-cost weight or None)
CONFIGS = [
    ("vel", 0x01, False, 0.0, False, None),
    ("vel_region", 0x01, False, 0.0, True, None),
    ("acc", 0x03, False, 0.0, False, None),
    ("acc_region", 0x03, False, 0.0, True, None),
    ("jrk", 0x07, False, 0.0, False, None),
    ("jrk_region", 0x07, False, 0.0, True, None),
    ("snp", 0x0F, False, 0.0, False, None),
    ("acc_pot", 0x03, True, 0.0, False, None),
    ("acc_pot_grad", 0x03, True, 0.25, False, None),
    ("accyaw_pot", 0x13, True, 0.0, False, 0.0),
    ("accyaw_pot_heading", 0x13, True, 0.25, False, 1.0),
    ("accyaw_pot_region", 0x13, True, 0.25, True, 0.0),
    ("accyaw_pot_region_heading", 0x13, True, 0.0, True, 1.0),
    ("jrkyaw_pot", 0x17, True, 0.25, False, 0.0),
    ("jrkyaw_pot_heading", 0x17, True, 0.0, False, 1.0),
    ("jrkyaw_pot_region", 0x17, True, 0.0, True, 0.0),
    ("jrkyaw_pot_region_heading", 0x17, True, 0.25, True, 1.0),
]
PAIR_CONFIGS = [c for c in CONFIGS if c[1] & 0x10]


def shape_id(dims):
    return "x".join(str(d) for d in dims)


WORLDS = [(dims, cfg) for dims in SHAPES for cfg in CONFIGS]
WORLD_IDS = ["%s-%s" % (shape_id(d), c[0]) for d, c in WORLDS]
PAIR_WORLDS = [(dims, cfg) for dims in SHAPES for cfg in PAIR_CONFIGS]
PAIR_IDS = ["%s-%s" % (shape_id(d), c[0]) for d, c in PAIR_WORLDS]


def world_name(dims, cfg):
    return "%s/%s" % (shape_id(dims), cfg[0])


def make_world(m, dims, cfg, n_nodes=N_NODES):
    name, control, potential, grad, region, wyaw = cfg
    # (the seed base is picked so that test (b)'s floors hold on all 136 worlds: with 500, say, the JRK world with a
    # search region on 33 x 40 x 96 has 26 finite successors)
    wl = _small_world(m, len(dims), control, seed=2500 + sum(dims) + control, n_nodes=n_nodes, potential=potential,
                      region=region, dims=dims)
    assert wl.map_dim == list(dims)
    if potential:
        wl.params["gradient_weight"] = grad
    if control & 0x10:
        wl.params["yaw_max"] = 0.9  # (a wide limit: a good share of the successors survives the heading test)
        wl.params["wyaw"] = wyaw
    return wl


def exchanged_env(wl, i, j):
    """The oracle's environment of wl with the SAME cells (map, potential, region) but axis lengths i and j exchanged:
    what a kernel computes that takes one axis length for the other."""
    md = list(wl.map_dim)
    md[i], md[j] = md[j], md[i]
    return O.Env(wl.dim, wl.control, wl.U, np.ascontiguousarray(wl.grid).ravel(), md, wl.origin, wl.res,
                 potential=None if wl.potential is None else np.ascontiguousarray(wl.potential).ravel(),
                 region=None if wl.region is None else np.ascontiguousarray(wl.region).ravel(), **wl.params)


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def _package():
    import motion_primitive_library_amd as m
    return m


def _changed_slots(a, b):
    return int(np.count_nonzero((a["status"] != b["status"]) | (a["hash"] != b["hash"]) | (a["iters"] != b["iters"]) |
                                (a["cost"].view(np.uint64) != b["cost"].view(np.uint64))))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_shapes_are_what_their_reasons_say():
    for dims in SHAPES:
        assert dims[0] % 4 != 0 or dims in ([80, 17, 33], [16, 48, 31]), dims
        assert len(set(dims)) == len(dims), dims
    assert int(np.prod(SHAPES[0])) % 2 == 1 and sorted(SHAPES[0]) == sorted(SHAPES[1]) and SHAPES[0] != SHAPES[1]
    assert SHAPES[2][0] % 32 == 16 and SHAPES[2][0] % 16 == 0 and SHAPES[3][0] * 2 == 32
    assert SHAPES[4][0] == 33 and SHAPES[7][0] == 33 and sorted(SHAPES[5]) == sorted(SHAPES[6])
    assert len(WORLDS) == 136


@pytest.mark.skipif(not os.path.exists(O.REF_SO), reason="oracle/_ref not built")
@pytest.mark.parametrize("dims,cfg", WORLDS, ids=WORLD_IDS)
def test_restatement_equals_the_reference_build(dims, cfg):
    """(a) status, hash, cost, iteration count and successor state, bit for bit."""
    wl = make_world(_package(), dims, cfg)
    a = O.expand(oracle_env(wl), wl.nodes, threads=4)
    b = O.expand(oracle_env(wl), wl.nodes, threads=4, ref=True)
    assert_slots_equal(a, b, cost_rtol=0.0, what=world_name(dims, cfg))
    assert a["stats"] == b["stats"]


@pytest.mark.parametrize("dims,cfg", WORLDS, ids=WORLD_IDS)
def test_worlds_discriminate_between_axis_lengths(dims, cfg):
    """(b) The precondition of everything below: every world has at least 50 finite (status 1) and 50 blocked (status
    2) successors, and an oracle given the same cells with two axis lengths exchanged -- every pair of axes -- changes
    at least 100 slots.  The floors are conditions on the inputs (seeds, node count), not tolerances; measured when the
    module was written: minima 68 finite, 164 blocked, 200 changed slots."""
    wl = make_world(_package(), dims, cfg)
    ref = O.expand(oracle_env(wl), wl.nodes, threads=4)
    st = ref["status"]
    n1, n2 = int(np.count_nonzero(st == 1)), int(np.count_nonzero(st == 2))
    changed = {}
    for i in range(wl.dim):
        for j in range(i + 1, wl.dim):
            changed[(i, j)] = _changed_slots(ref, O.expand(exchanged_env(wl, i, j), wl.nodes, threads=4))
    print("%s: %d finite, %d blocked, changed by an exchange %s" % (world_name(dims, cfg), n1, n2, changed))
    assert n1 >= 50 and n2 >= 50, (n1, n2)
    assert min(changed.values()) >= 100, changed
    # the border nodes of every axis: on the lower face, just below it, just inside the upper face, beyond it
    for i in range(wl.dim):
        assert wl.nodes[i, 4 * i:4 * i + 4].tolist() == [0.0, -0.03, dims[i] * wl.res - 0.01, dims[i] * wl.res + 0.2]


def test_geometry_fixture_is_complete_and_small():
    z = np.load(GOLDEN)
    assert sorted(str(n) for n in z["names"]) == sorted(world_name(d, c) for d, c in WORLDS)
    assert os.path.getsize(GOLDEN) <= 471237  # no larger than get_succ_golden.npz


@pytest.mark.parametrize("dims,cfg", WORLDS, ids=WORLD_IDS)
def test_oracle_reproduces_the_reference_made_fixture(dims, cfg):
    """(c) tests/golden/geometry_golden.npz holds what the reference build returned for these worlds
    (tests/golden/make_geometry_golden.py): dense status and iteration counts, SHA-256 of the hash and cost bytes.  It
    travels to machines without the reference build."""
    z = np.load(GOLDEN)
    name = world_name(dims, cfg)
    wl = make_world(_package(), dims, cfg)
    got = O.expand(oracle_env(wl), wl.nodes, threads=4)
    assert np.array_equal(digest(wl.nodes), z[name + "/nodes_sha256"]), "%s: the world's inputs changed" % name
    assert np.array_equal(digest(np.ascontiguousarray(wl.grid, dtype=np.int8)), z[name + "/grid_sha256"]), name
    assert np.array_equal(got["status"], z[name + "/status"]), name
    assert np.array_equal(got["iters"], z[name + "/iters"].astype(np.int32)), name
    assert np.array_equal(digest(got["hash"]), z[name + "/hash_sha256"]), name
    assert np.array_equal(digest(got["cost"]), z[name + "/cost_sha256"]), name


# ---------------------------------------------------------------------------------------------------------------- GPU
def _routes(cfg):
    """(route, kernel last_grid_kernel() must name) for every list route that covers the configuration: the tiled
    kernel takes neither yaw nor a potential map."""
    name, control, potential, grad, region, wyaw = cfg
    lex = not potential and control in (0x01, 0x03, 0x07)
    routes = [("grid", "lex" if lex else "grid")]
    if not potential and not control & 0x10:
        routes.append(("tile", "none"))
    routes.append(("dense", "none"))
    return routes


def _reference(wl, nodes=None):
    return O.expand(oracle_env(wl), wl.nodes if nodes is None else nodes, threads=8, ref=require_reference_build())


@pytest.mark.gpu
@pytest.mark.parametrize("dims,cfg", WORLDS, ids=WORLD_IDS)
def test_lists_on_every_route_equal_the_reference(engine, dims, cfg):
    """(d) count, order, action, hash, state and iteration count bit for bit; cost bit for bit without yaw, within the
    north-star tolerance with yaw (device cos / sin against the host's)."""
    wl = make_world(engine, dims, cfg)
    ref = _reference(wl)
    rtol = YAW_COST_RTOL if cfg[1] & 0x10 else 0.0
    env = engine_env(engine, wl)
    for route, kernel in _routes(cfg):
        env.set_lists_route(route)
        got = env.expand_lists(wl.nodes)
        assert env.last_lists_route() == route, (route, env.last_lists_route())  # a route that refused would show here
        assert env.last_grid_kernel() == kernel, (route, env.last_grid_kernel())
        assert_lists_equal(got, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=rtol,
                           what="%s route %s" % (world_name(dims, cfg), route))
    if cfg[2] or cfg[1] & 0x10:  # the tiled kernel does not cover these: asking for it is an error, not another kernel
        env.set_lists_route("tile")
        with pytest.raises(engine._abi.MplxError):
            env.expand_lists(wl.nodes)
    env.set_lists_route("auto")
    got = env.expand_lists(wl.nodes)
    assert env.last_lists_route() == "grid"
    assert_lists_equal(got, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=rtol, what="%s route auto" % world_name(dims, cfg))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dims", SHAPES, ids=[shape_id(d) for d in SHAPES])
@pytest.mark.parametrize("cfg", [CONFIGS[2], CONFIGS[7]], ids=["acc", "acc_pot"])
def test_resident_launch_of_a_large_frontier(engine, dims, cfg):
    """(d) A resident launch of the frontier tiled to 5 120 nodes: the size at which the free-box (summed-area) table
    is in use for most of the frontier, on occupancy (lex kernel) and on a potential map (general kernel)."""
    wl = make_world(engine, dims, cfg)
    big = np.ascontiguousarray(np.tile(wl.nodes, (1, 32)))
    assert big.shape[1] >= 5000
    ref = _reference(wl, big)
    env = engine_env(engine, wl)
    env.set_lists_route("grid")
    fr = env.upload_frontier(big)
    lists = env.alloc_lists(big.shape[1], want_state=True, want_iters=True)
    env.expand_lists_resident(fr, lists)
    env.synchronize()
    got = lists.download()
    assert env.last_lists_route() == "grid" and env.last_grid_kernel() == ("grid" if cfg[2] else "lex")
    lists.free()
    fr.free()
    env.close()
    assert_lists_equal(got, ref, big.shape[1], wl.U.shape[0], what="%s, %d nodes resident" % (world_name(dims, cfg), big.shape[1]))


@pytest.mark.gpu
@pytest.mark.parametrize("dims,cfg", PAIR_WORLDS, ids=PAIR_IDS)
def test_pair_kernel_equals_the_reference_and_the_general_kernel(engine, monkeypatch, dims, cfg):
    """(d, e) Yaw controls on a potential map over a pre-screened frontier: expand_pair_kernel against the reference, and
    against the general factorised kernel (MPLX_GRID_PAIR=0) on everything bit for bit, costs included."""
    from test_gpu_pair import _lists, _same_lists
    wl = make_world(engine, dims, cfg)
    ref = _reference(wl)
    got, kernel = _lists(engine, wl, monkeypatch, pair=True)
    assert kernel == "pair", kernel
    what = world_name(dims, cfg)
    assert_lists_equal(got, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=YAW_COST_RTOL, what=what + " pair")
    gen, kernel = _lists(engine, wl, monkeypatch, pair=False)
    assert kernel == "grid", kernel
    assert_lists_equal(gen, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=YAW_COST_RTOL, what=what + " pre-screened general")
    _same_lists(got, gen, wl.n_nodes, what + " pair vs general")


ODD_DIMS = {2: [53, 37], 3: [29, 53, 37]}  # for helpers.odd_world: nothing round in the map shape either


def _odd(m, seed):
    return odd_world(m, seed, N_NODES, dims=ODD_DIMS[2 + seed % 2])


@pytest.mark.parametrize("seed", range(16))
def test_odd_worlds_on_a_non_cube_discriminate_and_equal_the_reference_build(seed):
    """(a, b) for the worlds with odd resolutions, durations, origins off the lattice and control values like 1/3."""
    wl, control, pot = _odd(_package(), seed)
    ref = O.expand(oracle_env(wl), wl.nodes, threads=4)
    st = ref["status"]
    assert np.count_nonzero(st == 1) >= 50 and np.count_nonzero(st == 2) >= 50, np.bincount(st, minlength=4)
    for i in range(wl.dim):
        for j in range(i + 1, wl.dim):
            assert _changed_slots(ref, O.expand(exchanged_env(wl, i, j), wl.nodes, threads=4)) >= 100, (i, j)
    if os.path.exists(O.REF_SO):
        assert_slots_equal(ref, O.expand(oracle_env(wl), wl.nodes, threads=4, ref=True), what="odd world %d" % seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(16))
def test_odd_worlds_on_a_non_cube_all_routes(engine, seed):
    """(d) as tests/test_gpu_lists.py::test_irregular_parameters_all_routes, on maps whose axes differ."""
    wl, control, pot = _odd(engine, seed)
    ref = _reference(wl)
    env = engine_env(engine, wl)
    rtol = YAW_COST_RTOL if control & 0x10 else 0.0
    routes = ["auto", "dense"] + (["tile"] if not (control & 0x10) and pot is None else [])
    seen = set()
    for route in routes:
        env.set_lists_route(route)
        got = env.expand_lists(wl.nodes)
        seen.add(env.last_lists_route())
        assert route == "auto" or env.last_lists_route() == route
        assert_lists_equal(got, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=rtol, what="odd world %d on %s, route %s (%s)" % (
            seed, shape_id(wl.map_dim), route, env.last_lists_route()))
    env.close()
    assert "dense" in seen and (control == 0x1F or "grid" in seen or control == 0x0F and pot is not None), seen


def _edges(m, dims, control, region):
    from test_edges import _edges as edges
    return edges(m, len(dims), control, 7300 + sum(dims) + control, region, dims=dims)


@pytest.mark.parametrize("dims", SHAPES, ids=[shape_id(d) for d in SHAPES])
@pytest.mark.parametrize("control", [0x03, 0x07])
def test_edge_worlds_discriminate_between_axis_lengths(dims, control):
    """The edge kernel's precondition, as (b): at least 20 free and 20 blocked edges among the 400, and an exchange of
    any two axis lengths changes the answer (free flag or the cells walked) of at least 200 of them.  Conditions on the
    inputs, not tolerances; measured when the module was written: minima 22 free, 202 blocked, 394 changed."""
    for region in (False, True):
        wl, actions = _edges(_package(), dims, control, region)
        a = O.check_edges(oracle_env(wl), wl.nodes, actions, cell_cap=64)
        assert 20 <= a["free"].sum() <= actions.size - 20, a["free"].sum()
        for i in range(wl.dim):
            for j in range(i + 1, wl.dim):
                b = O.check_edges(exchanged_env(wl, i, j), wl.nodes, actions, cell_cap=64)
                diff = (a["free"] != b["free"]) | (a["cell_count"] != b["cell_count"]) | (a["cells"] != b["cells"]).any(axis=1)
                assert np.count_nonzero(diff) >= 200, (i, j, np.count_nonzero(diff))


@pytest.mark.skipif(not os.path.exists(O.REF_SO), reason="oracle/_ref not built")
@pytest.mark.parametrize("dims", SHAPES, ids=[shape_id(d) for d in SHAPES])
@pytest.mark.parametrize("control", [0x03, 0x07])
def test_edge_restatement_equals_the_reference_build(dims, control):
    for region in (False, True):
        wl, actions = _edges(_package(), dims, control, region)
        a = O.check_edges(oracle_env(wl), wl.nodes, actions, cell_cap=64)
        b = O.check_edges(oracle_env(wl), wl.nodes, actions, cell_cap=64, ref=True)
        assert np.array_equal(a["free"], b["free"]) and np.array_equal(a["cost"], b["cost"])
        assert np.array_equal(a["cell_count"], b["cell_count"]) and a["cell_count"].max() <= 64
        for k in range(actions.size):
            c = a["cell_count"][k]
            assert np.array_equal(a["cells"][k, :c], b["cells"][k, :c]), k


@pytest.mark.gpu
@pytest.mark.parametrize("dims", SHAPES, ids=[shape_id(d) for d in SHAPES])
@pytest.mark.parametrize("control", [0x03, 0x07])
@pytest.mark.parametrize("region", [False, True])
def test_device_edges_match_the_oracle(engine, dims, control, region):
    """(f) edge_kernel through check_edges: free flag, cost, the cells walked (cell_cap 64, truncated to 3, none)."""
    wl, actions = _edges(engine, dims, control, region)
    env = engine_env(engine, wl)
    got = env.check_edges(wl.nodes, actions, cell_cap=64)
    small = env.check_edges(wl.nodes, actions, cell_cap=3)   # truncated rows still report the full count
    plain = env.check_edges(wl.nodes, actions)
    env.close()
    ref = O.check_edges(oracle_env(wl), wl.nodes, actions, cell_cap=64, ref=require_reference_build())
    assert np.array_equal(got["free"], ref["free"]) and np.array_equal(plain["free"], ref["free"])
    assert np.array_equal(got["cost"], ref["cost"]) and np.array_equal(plain["cost"], ref["cost"])
    assert np.array_equal(got["cell_count"], ref["cell_count"]) and np.array_equal(small["cell_count"], ref["cell_count"])
    for k in range(actions.size):
        c = ref["cell_count"][k]
        assert np.array_equal(got["cells"][k, :c], ref["cells"][k, :c]), k
        assert np.array_equal(small["cells"][k, :min(c, 3)], ref["cells"][k, :min(c, 3)]), k
    assert (ref["free"][:4] == 0).all() and np.isinf(ref["cost"][:4]).all()  # the edges that do not move


@pytest.mark.gpu
@pytest.mark.parametrize("dims", [[53, 37, 29], [75, 43]], ids=["53x37x29", "75x43"])
def test_map_preparation_feeds_the_expansion_on_a_non_cube(engine, dims):
    """(g) updatePotentialMap and setSearchRegion, then dilate(box), then editMap of a few cells, then expand_lists --
    against the oracle fed with O.update_potential_map, O.search_region and np_dilate.  While the potential map is
    installed the expansion reads that copy alone (env_map.h:113-120): the dilate and the edit change the MapUtil's
    map, not the lists.  With the potential map taken away the expansion reads the dilated, edited map; a second edit
    and a frontier of 5 120 nodes then rebuild the free-box table from the patched bits."""
    from test_map_util import box, np_dilate
    dim = len(dims)
    wl = make_world(engine, dims, CONFIGS[2])  # ACC on occupancy
    md, org, res = wl.map_dim, wl.origin, wl.res
    nU = wl.U.shape[0]
    radius = [0.4, 0.3, 0.5][:dim]
    path = np.array([[0.5] * dim, [md[i] * res * 0.5 for i in range(dim)], [md[i] * res - 0.5 for i in range(dim)]])
    path[1, 0] += 0.7  # (a bend: the tunnel is not the diagonal's)
    sr = [1.0, 0.8, 0.9][:dim]
    kw = dict(wl.params)
    kw.update(potential_weight=0.5, gradient_weight=0.25)
    env = engine_env(engine, wl)
    env.set_potential_weight(0.5)
    env.set_gradient_weight(0.25)
    pot = env.updatePotentialMap([0.0] * dim, radius)
    reg = env.setSearchRegion(path, sr)
    want_pot = O.update_potential_map(wl.grid, md, org, res, [0.0] * dim, radius)
    want_reg = O.search_region(md, org, res, path, sr)
    assert np.array_equal(pot, want_pot) and np.array_equal(reg, want_reg)
    assert 0 < np.count_nonzero(want_reg) < want_reg.size and np.count_nonzero((want_pot > 0) & (want_pot < 100)) > 500
    got_map = env.dilate(box(dim))
    dil = np_dilate(want_pot, md, box(dim))
    assert np.array_equal(got_map, dil) and not np.array_equal(dil, want_pot)
    rng = np.random.default_rng(sum(dims))
    occ, free = np.nonzero(dil == 100)[0], np.nonzero(dil != 100)[0]
    idx = np.concatenate([rng.choice(free, 300, replace=False), rng.choice(occ, 300, replace=False), [0, dil.size - 1]])
    val = np.concatenate([np.full(300, 100, np.int8), np.zeros(300, np.int8), [100, 100]]).astype(np.int8)
    env.editMap(idx, val)
    edited = dil.copy()
    edited[idx] = val
    assert np.array_equal(env.read_cells(np.arange(dil.size)), edited)
    assert np.array_equal(env.read_cells(np.arange(dil.size), potential=True), want_pot)
    # with the potential map installed
    oenv = O.Env(dim, wl.control, wl.U, want_pot, md, org, res, potential=want_pot, region=want_reg, **kw)
    ref = O.expand(oenv, wl.nodes, threads=8)
    assert np.count_nonzero(ref["status"] == 1) >= 50 and np.count_nonzero(ref["status"] == 2) >= 50
    for route in ("grid", "dense"):
        env.set_lists_route(route)
        got = env.expand_lists(wl.nodes)
        assert env.last_lists_route() == route
        assert_lists_equal(got, ref, wl.n_nodes, nU, what="%s prepared potential + region, route %s" % (shape_id(dims), route))
    # without it: the dilated, edited map under the device-made region
    env.set_potential_map(None)
    oenv2 = O.Env(dim, wl.control, wl.U, edited, md, org, res, region=want_reg, **kw)
    ref2 = O.expand(oenv2, wl.nodes, threads=8)
    assert np.count_nonzero(ref2["status"] == 1) >= 50 and np.count_nonzero(ref2["status"] == 2) >= 50
    assert _changed_slots(ref, ref2) >= 100
    for route, kernel in (("grid", "lex"), ("tile", "none"), ("dense", "none")):
        env.set_lists_route(route)
        got = env.expand_lists(wl.nodes)
        assert env.last_lists_route() == route and env.last_grid_kernel() == kernel
        assert_lists_equal(got, ref2, wl.n_nodes, nU, what="%s dilated + edited map, route %s" % (shape_id(dims), route))
    idx2 = rng.choice(np.nonzero(edited == 100)[0], 200, replace=False)
    env.editMap(idx2, np.zeros(200, np.int8))
    edited[idx2] = 0
    big = np.ascontiguousarray(np.tile(wl.nodes, (1, 32)))
    oenv3 = O.Env(dim, wl.control, wl.U, edited, md, org, res, region=want_reg, **kw)
    env.set_lists_route("grid")
    got_big = env.expand_lists(big)
    assert env.last_grid_kernel() == "lex"
    assert_lists_equal(got_big, O.expand(oenv3, big, threads=8), big.shape[1], nU,
                       what="%s second edit, %d nodes (free-box table rebuilt)" % (shape_id(dims), big.shape[1]))
    env.close()
