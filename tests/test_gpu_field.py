"""GPU: include/mplx_field.h against tests/field_model.py -- the field on every cell (==) on maps built to hit the tiling,
staleness and every error of the header, the push with a field byte for byte, the admissibility of the heuristic against
the plain search's optimal costs, and the search that uses it (search / search_many / plan_prioritised / replan)."""
import numpy as np
import pytest

import control_matrix as CM
import field_model as FM

pytestmark = pytest.mark.gpu

POISON = 0xAB


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def code(m, fn):
    with pytest.raises(m._abi.MplxError) as e:
        fn()
    return e.value.code


def map_env(m, dims, cells, res=1.0, origin=None, control=None, vals=(-1.0, 0.0, 1.0), v_max=1.0, yaw=False):
    D = len(dims)
    env = m.EnvMap(D)
    env.setMap([0.0] * D if origin is None else origin, list(dims), np.asarray(cells, np.int8).ravel(), res)
    env.set_control(m.ACC if control is None else control)
    env.set_u(m.workloads.grid_controls(list(vals), D, yaw_rates=[-0.3, 0.0, 0.3]) if yaw else m.workloads.grid_controls(list(vals), D))
    env.set_v_max(v_max)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    if yaw:
        env.set_yaw_max(0.5)
    return env


# ------------------------------------------------------------------------------------------------------ the field
def random_map(seed, dims, share):
    """Blocked with probability `share`, and a wall across axis 0 at its middle with one gap in the far corner, so that
    the cells behind it are further away than their Chebyshev distance."""
    rng = np.random.default_rng(seed)
    shape = tuple(reversed(dims))  # [z][y][x]
    c = np.where(rng.random(shape) < share, 100, 0).astype(np.int8)
    mid = dims[0] // 2
    c[..., mid] = 100
    gap = tuple(s - 1 for s in shape[:-1])
    c[gap + (mid,)] = 0
    return c.ravel()


def spiral_map(n=67):
    """Concentric square walls one cell thick, two cells apart, each with one gap, the gaps on alternating sides: the
    only route from the rim to the centre runs half way round every ring, through every tile several times."""
    c = np.zeros((n, n), np.int8)
    mid = n // 2
    for k in range(1, mid - 1, 2):
        c[k, k:n - k] = c[n - 1 - k, k:n - k] = 100
        c[k:n - k, k] = c[k:n - k, n - 1 - k] = 100
        c[mid, k if (k // 2) % 2 == 0 else n - 1 - k] = 0
    return c.ravel()


def boxes(seed, dims, F):
    """F seed boxes: the first in the corner (0, ..), then random ones, some clipped by the map's edge, one wholly outside."""
    rng = np.random.default_rng(seed)
    D = len(dims)
    lo, hi = [[0] * D], [[1] * D]
    for f in range(1, F):
        a = [int(rng.integers(-2, dims[i])) for i in range(D)]
        lo.append(a)
        hi.append([a[i] + int(rng.integers(0, 3)) for i in range(D)])
    if F > 2:
        lo[2], hi[2] = [dims[i] + 1 for i in range(D)], [dims[i] + 3 for i in range(D)]
    return lo, hi


def band_region(dims):
    """A search region: everything but a band of rows near the top (which is outside)."""
    r = np.ones(tuple(reversed(dims)), np.uint8)
    r[..., -4:-2, :] = 0
    r[..., -4:-2, :3] = 1  # (a passage through the band)
    return r.ravel()


def potential_of(seed, dims):
    """A quarter of the cells cost (1 .. 99), a seventh block (100 .. 127); a blocking wall with a gap of cost cells."""
    rng = np.random.default_rng(seed)
    shape = tuple(reversed(dims))
    p = np.where(rng.random(shape) < 0.25, rng.integers(1, 100, size=shape), 0)
    p = np.where(rng.random(shape) < 0.15, rng.integers(100, 128, size=shape), p).astype(np.int8)
    mid = dims[0] // 2
    p[..., mid] = 110
    p[tuple(s - 1 for s in shape[:-1]) + (mid,)] = 99
    return p.ravel()


FIELD_CASES = {
    "2d-37x29-F1-corner": dict(dims=[37, 29], share=0.2, F=1),
    "2d-70x33-F3": dict(dims=[70, 33], share=0.2, F=3),
    "2d-70x33-F65-dense": dict(dims=[70, 33], share=0.45, F=65),
    "3d-19x13x11-F1": dict(dims=[19, 13, 11], share=0.2, F=1),
    "3d-9x17x8-F3-dense": dict(dims=[9, 17, 8], share=0.45, F=3),
    "3d-19x13x11-F65": dict(dims=[19, 13, 11], share=0.2, F=65),
    "2d-67x67-spiral": dict(dims=[67, 67], spiral=True, F=1),
    "2d-37x29-region": dict(dims=[37, 29], share=0.2, F=3, region=True),
    "2d-70x33-potential": dict(dims=[70, 33], share=0.2, F=1, potential=True),
}


@pytest.mark.parametrize("name", sorted(FIELD_CASES))
def test_field_equals_the_model(engine, name):
    m, case = engine, FIELD_CASES[name]
    dims, F = case["dims"], case["F"]
    seed = sum(dims) + F
    cells = spiral_map(dims[0]) if case.get("spiral") else random_map(seed, dims, case["share"])
    if case.get("spiral"):
        lo, hi = [[dims[0] // 2, dims[1] // 2]], [[dims[0] // 2, dims[1] // 2]]
    else:
        lo, hi = boxes(seed, dims, F)
    region = band_region(dims) if case.get("region") else None
    pot = potential_of(seed, dims) if case.get("potential") else None
    want = FM.field(FM.blocked_of(cells, region, pot), dims, lo, hi)
    if pot is not None:  # cost cells (1 .. 99) are traversable: the field is not the one of "value > 0 blocks"
        assert (pot >= 100).any() and ((pot > 0) & (pot < 100)).any()
        assert not np.array_equal(want, FM.field(pot > 0, dims, lo, hi))
    # what the case is there for, on the model alone
    cheb = np.stack([FM.chebyshev_to_box(dims, lo[f], hi[f]) for f in range(F)])
    unreachable, detour = (want < 0).mean(), ((want >= 0) & (want > cheb)).mean()
    print("%s: -1 share %.3f, dist > Chebyshev share %.3f, largest dist %d" % (name, unreachable, detour, want.max()))
    assert unreachable > 0 and detour > 0
    assert np.all(want[want >= 0] >= cheb[want >= 0])
    ts = 32 if len(dims) == 2 else 8
    n_tiles = int(np.prod([(d + ts - 1) // ts for d in dims]))
    assert n_tiles > 1 and any(d % ts for d in dims)
    if case.get("spiral"):
        # a tile of 32 x 32 holds an L-shaped piece of a ring of at most 63 cells, so the route enters tiles at least
        # max / 64 times: more often than there are tiles
        assert want.max() // 64 > n_tiles, (want.max(), n_tiles)
    env = map_env(m, dims, cells)
    if region is not None:
        env.set_search_region(region)
    if pot is not None:
        env.set_potential_map(pot)
    fld = env.alloc_field()
    assert fld.shape == (0, 0) and not fld.stale
    fld.build_boxes(lo, hi)
    got = fld.dist()
    print("passes", fld.passes, "tiles", n_tiles)
    assert fld.shape == (F, int(np.prod(dims))) and not fld.stale
    assert got.dtype == np.int32 and np.array_equal(got, want)
    fld.build_boxes(lo, hi)  # the same build twice: the same bytes
    assert got.tobytes() == fld.dist().tobytes()
    fld.free()
    env.close()


def test_staleness_errors_and_limits(engine):
    m = engine
    A = m._abi
    L = A.lib()
    dims = [37, 29]
    cells = random_map(5, dims, 0.2)
    env = map_env(m, dims, cells)
    F = env.n_fields
    lo, hi = boxes(5, dims, 3)
    fld = env.alloc_field().build_boxes(lo, hi)
    goal = np.zeros(F)
    goal[:2] = [30.5, 20.5]
    tab = env.alloc_table(64)
    opn = env.alloc_open(tab)
    st = np.zeros((F, 2))
    st[:2] = [[3.5, 4.5], [3.5, 5.5]]
    fr = m.TableFrontier(env, 2)
    raw_set = lambda o, f, q: A.check(env._ctx, L.mplx_open_set_field(o, f, q))
    # ---- set_field's errors
    assert code(m, lambda: opn.set_field(fld, [0])) == A.ERR_STATE                   # no goal yet
    env.set_goal(goal, tol_pos=0.5)
    assert tab.seed(st, frontier=fr) == 2
    assert code(m, lambda: raw_set(opn._open, None, None)) == A.ERR_ARG
    assert code(m, lambda: opn.set_field(fld, [3])) == A.ERR_ARG and code(m, lambda: opn.set_field(fld, [-2])) == A.ERR_ARG
    empty = env.alloc_field()
    assert code(m, lambda: opn.set_field(empty, [0])) == A.ERR_STATE                 # an empty field
    empty.build_boxes(np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32))        # F == 0: a no-op that leaves it empty
    assert empty.shape == (0, 0) and empty.dist().shape == (0, 0)
    other = map_env(m, dims, cells)
    fld_o = other.alloc_field().build_boxes(lo, hi)
    assert code(m, lambda: opn.set_field(fld_o, [0])) == A.ERR_ARG                   # a field of another context
    fld_o.free()
    other.close()
    env.set_goal(goal, tol_pos=0.5, v_max=0.0)
    assert code(m, lambda: opn.set_field(fld, [0])) == A.ERR_STATE                   # v_max <= 0
    env.set_goal(goal, tol_pos=0.5)
    opn.set_field(fld, [0])
    env.set_goal(goal, tol_pos=0.5, v_max=-1.0)
    assert code(m, lambda: opn.push(fr, n_max=2)) == A.ERR_STATE                     # ... also when the goal changes under it
    env.set_goal(goal, tol_pos=0.5)
    # ---- a field together with priors, whichever is set second
    tab1 = env.alloc_table(64)
    opn1 = env.alloc_open(tab1)
    opn1.set_goals(goal.reshape(1, -1), tol_pos=0.5)
    U = np.asarray(m.workloads.grid_controls([-1.0, 0.0, 1.0], 2))
    opn1.set_field(fld, [1])
    assert code(m, lambda: opn1.set_priors(st[:, :1], np.array([[4], [4]], np.int32), m.ACC, U, 1.0)) == A.ERR_STATE
    opn1.clear_field()
    opn1.set_priors(st[:, :1], np.array([[4], [4]], np.int32), m.ACC, U, 1.0)
    assert code(m, lambda: opn1.set_field(fld, [1])) == A.ERR_STATE
    opn1.set_goals(goal.reshape(1, -1), tol_pos=0.5)                                 # drops the priors
    opn1.set_field(fld, [1])
    opn1.set_goals(goal.reshape(1, -1), tol_pos=0.5)                                 # ... and the field
    opn1.set_priors(st[:, :1], np.array([[4], [4]], np.int32), m.ACC, U, 1.0)
    opn1.free()
    tab1.free()
    # ---- a push with the field works, survives clear(), and is refused once the map was edited
    opn.push(fr, n_max=2)
    opn.clear()
    opn.push(fr, n_max=2)
    cell = 7 + 37 * 9
    new = cells.copy()
    new[cell] = 0 if cells[cell] else 100
    assert not fld.stale
    env.editMap([cell], [new[cell]])
    assert fld.stale
    assert code(m, lambda: opn.push(fr, n_max=2)) == A.ERR_STATE
    assert code(m, lambda: opn.push(fr, n_max=2, closed=True)) == A.ERR_STATE
    fld.build_boxes(lo, hi)
    assert not fld.stale and np.array_equal(fld.dist(), FM.field(FM.blocked_of(new), dims, lo, hi))
    opn.push(fr, n_max=2)
    # a rebuild with fewer fields than the queries use
    opn.set_field(fld, [2])
    fld.build_boxes(lo[:1], hi[:1])
    assert code(m, lambda: opn.push(fr, n_max=2)) == A.ERR_STATE
    # the other calls that can change a blocked bit
    for change in (lambda: env.set_search_region(band_region(dims)), lambda: env.set_search_region(None),
                   lambda: env.set_potential_map(potential_of(1, dims)), lambda: env.set_potential_map(None),
                   lambda: env.setMap([0.0, 0.0], dims, new, 1.0), lambda: env.freeUnknown(read_back=False)):
        fld.build_boxes(lo, hi)
        assert not fld.stale
        change()
        assert fld.stale
    # ---- build's errors
    raw_build = lambda f, n, a, b: A.check(env._ctx, L.mplx_field_build(f, n, a, b))
    z = np.zeros(2, np.int32)
    assert code(m, lambda: raw_build(fld._fld, -1, z.ctypes.data, z.ctypes.data)) == A.ERR_ARG
    assert code(m, lambda: raw_build(fld._fld, 1, None, z.ctypes.data)) == A.ERR_ARG
    too_many = A.FIELD_MAX_BYTES // 4 // (37 * 29) + 1
    assert code(m, lambda: raw_build(fld._fld, too_many, z.ctypes.data, z.ctypes.data)) == A.ERR_ARG   # (checked before the boxes are read)
    assert code(m, lambda: A.check(env._ctx, L.mplx_field_view_of(fld._fld, None))) == A.ERR_ARG
    bare = m.EnvMap(2)
    f_bare = bare.alloc_field()
    assert code(m, lambda: A.check(bare._ctx, L.mplx_field_build(f_bare._fld, 1, z.ctypes.data, z.ctypes.data))) == A.ERR_STATE  # no map
    f_bare.free()
    bare.close()
    with pytest.raises(ValueError):
        env.search(st[:, 0], goal, field=True, prior=m.search.Prior(st[:, 0], [4], m.ACC, U, 1.0))
    # ---- a field destroyed while in force: the next push is an error, until the open set is told otherwise
    env.setMap([0.0, 0.0], dims, new, 1.0)
    gone = env.alloc_field().build_boxes(lo, hi)
    opn.set_field(gone, [0])
    opn.push(fr, n_max=2)
    gone.free()
    assert code(m, lambda: opn.push(fr, n_max=2)) == A.ERR_STATE
    opn.clear_field()
    opn.push(fr, n_max=2)
    fld.build_boxes(lo, hi)
    opn.set_field(fld, [0])
    again = env.alloc_field().build_boxes(lo, hi)
    opn.set_field(again, [1])   # replaces fld, which may go now
    fld.free()
    opn.push(fr, n_max=2)
    opn.free()                  # ... and an open set that goes first leaves the field alone
    again.free()
    env.synchronize()
    for b in (empty, fr, tab):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ the push
def push_world(D):
    """A wall across x with a gap at the far end of the other axes, a sealed pocket, and rows of every kind."""
    dims = [20, 16] if D == 2 else [12, 10, 7]
    res = 0.5
    shape = tuple(reversed(dims))
    c = np.zeros(shape, np.int8)
    wall = dims[0] // 2
    c[..., wall] = 100
    c[tuple(s - 1 for s in shape[:-1]) + (wall,)] = 0
    # a pocket: the free cell (2, 2[, 2]) inside a closed box
    box = tuple(slice(1, 4) for _ in range(D))
    c[box] = 100
    c[(2,) * D] = 0
    return dims, res, c.ravel()


def push_rows(D, dims, res, goals, n_fields, yaw, order, foq):
    """States [4D+2][n] and their queries: per query a lattice of cell centres on both sides of the wall (a sparse one for
    a query that keeps the default heuristic), the goal row itself, rows inside the goal box, the pocket, a blocked cell,
    and positions off the map."""
    rng = np.random.default_rng(11 * D + order)
    Q = len(goals)
    cols, query = [], []
    for q in range(Q):
        pts = []
        sx, sy = (2, 3 if D == 2 else 2) if foq[q] >= 0 else (4, 6)
        for x in range(0, dims[0], sx):
            for y in range(0, dims[1], sy):
                p = [(x + 0.5) * res + 0.01 * q, (y + 0.5) * res]
                if D == 3:
                    p.append((((x + y) % dims[2]) + 0.5) * res)
                pts.append(p)
        g = goals[q][:D]
        pts += [list(g), list(g + 0.2), list(g - 0.3)]                              # the goal state, inside the box
        pts += [[(2 + 0.5) * res + 0.01 * q] + [(2 + 0.5) * res] * (D - 1)]         # the pocket
        pts += [[(dims[0] // 2 + 0.5) * res + 0.01 * q] + [1.5 * res] * (D - 1)]    # on the wall
        pts += [[-0.3 - 0.01 * q] + [1.0] * (D - 1), [1.0 + 0.01 * q] + [dims[1] * res + 0.2] + [1.0] * (D - 2)]  # off the map
        for j, p in enumerate(pts):
            s = np.zeros(n_fields)
            s[:D] = p
            is_goal = j == len(pts) - 7
            if order >= 2 and not is_goal:
                s[D:2 * D] = rng.choice([-0.5, 0.0, 0.5], size=D)
            if order >= 3 and not is_goal:
                s[2 * D:3 * D] = rng.choice([-0.5, 0.0, 0.25], size=D)
            if order >= 4 and not is_goal:
                s[3 * D:4 * D] = rng.choice([-0.3, 0.0, 0.6], size=D)
            if yaw and not is_goal:
                s[4 * D] = rng.choice([0.0, 0.1, -0.2])
            cols.append(s)
            query.append(q)
    return np.stack(cols, axis=1), np.array(query, np.int32)


PUSH_CASES = [(2, "VEL", 1), (2, "ACC", 3), (2, "ACCxYAW", 3), (3, "VEL", 3), (3, "ACC", 1), (3, "ACCxYAW", 1)]
PUSH_CASES = PUSH_CASES + CM.PUSH_ADDED  # SNP and JRKxYAW: rows with live acc and jerk (tests/control_matrix.py)


@pytest.mark.parametrize("D,control,Q", PUSH_CASES, ids=["%dd-%s-Q%d" % c for c in PUSH_CASES])
def test_push_equals_the_model(engine, D, control, Q):
    m = engine
    yaw = control.endswith("YAW")
    order = CM.order_of(control)
    dims, res, cells = push_world(D)
    W, VMAX = 10.0, 2.0
    env = map_env(m, dims, cells, res=res, control=getattr(m, control), vals=(-0.5, 0.0, 0.5), v_max=VMAX, yaw=yaw)
    F = env.n_fields
    org = [0.0] * D
    # goals on the far side of the wall, low; query 0 -> field 1, query 1 -> the default heuristic, query 2 -> field 0
    goal_pos = [[(dims[0] - 3 + 0.5) * res] + [1.5 * res] * (D - 1), [(dims[0] - 2 + 0.5) * res] + [2.5 * res] * (D - 1),
                [(dims[0] - 3 + 0.5) * res] + [3.5 * res] * (D - 1)][:Q]
    goals = np.zeros((Q, F))
    goals[:, :D] = goal_pos
    foq = [1, -1, 0][:Q]
    field_goal = [2, 0] if Q == 3 else [0, 0]   # field 0 belongs to the goal of query 2, field 1 to that of query 0
    blo, bhi = zip(*[FM.goal_box(goals[q][:D], 0.5, org, res) for q in field_goal])
    fld = env.alloc_field().build(goals[field_goal], 0.5)
    dist = fld.dist()
    assert np.array_equal(dist, FM.field(FM.blocked_of(cells), dims, blo, bhi))
    states, query = push_rows(D, dims, res, goals, F, yaw, order, foq)
    n = states.shape[1]
    g = 0.25 * np.arange(n)
    tab = env.alloc_table(1024, n_queries=Q)
    opn = env.alloc_open(tab)
    if Q > 1:
        opn.set_goals(goals, w=W, v_max=VMAX, tol_pos=0.5)
    else:
        env.set_goal(goals[0], w=W, v_max=VMAX, tol_pos=0.5)
    fr = m.TableFrontier(env, n)
    assert tab.seed(states, g, frontier=fr, query=query if Q > 1 else None) == n      # node k = seed k
    d = tab.download()
    assert d["n_nodes"] == n and np.array_equal(bits(d["state"][:D]), bits(states[:D])) and np.array_equal(fr.download()["id"], np.arange(n))
    goal_hash = [d["hash"][np.nonzero((query == q) & np.all(states[:D].T == goals[q][:D], axis=1))[0][0]] for q in range(Q)]
    # ---- the model, row by row
    kinds = {"G>L": 0, "G<=L": 0, "inf": 0, "goal": 0, "default": 0, "off": 0, "inside": 0}
    h_field, h_plain = np.zeros(n), np.zeros(n)
    for k in range(n):
        q = int(query[k])
        is_goal = d["hash"][k] == goal_hash[q]
        h_plain[k] = FM.default_heuristic(states[:D, k], goals[q], W, VMAX, D, is_goal)
        if foq[q] < 0:
            h_field[k] = h_plain[k]
            kinds["default"] += 1
            continue
        h, G, L = FM.heuristic(states[:D, k], goals[q], W, VMAX, dist[foq[q]], dims, org, res, is_goal)
        h_field[k] = h
        c = FM.cell_of(states[:D, k], dims, org, res)
        kinds["goal" if is_goal else "inf" if G is None else "G>L" if G > L else "G<=L"] += 1
        kinds["off"] += c is None and not is_goal
        kinds["inside"] += c is not None and dist[foq[q]][c] == 0
    print(control, D, Q, kinds, "of", n)
    assert kinds["G>L"] >= n / 4 and kinds["G<=L"] >= n / 4  # of ALL rows, those of a query without a field included
    assert kinds["goal"] >= 1 and kinds["inf"] >= 3 and kinds["off"] >= 2 and kinds["inside"] >= 3

    cap = opn.capacity
    v = opn.view()

    def pushed(eps, sight, closed, n_max):
        opn.clear()
        env.synchronize()
        A = m._abi
        A.check(env._ctx, A.lib().mplx_memset(env._ctx, v.f, POISON, cap * 8))
        A.check(env._ctx, A.lib().mplx_memset(env._ctx, v.flags, POISON, cap))
        opn.push(fr, n_max=n_max, eps=eps, sight=sight, closed=closed)
        env.synchronize()
        return tab._read(v.f, np.uint64, cap), tab._read(v.flags, np.uint8, cap)

    n_max = n - 2  # the last two rows stay behind n_max
    for eps, sight, closed in ((1.0, False, False), (2.0, False, True), (1.0, True, False), (0.5, True, True)):
        f0, fl0 = pushed(eps, sight, closed, n_max)
        opn.set_field(fld, foq)
        f1, fl1 = pushed(eps, sight, closed, n_max)
        opn.clear_field()
        f2, fl2 = pushed(eps, sight, closed, n_max)
        want0 = np.array([FM.key(g[k], eps, h_plain[k]) for k in range(n_max)]).view(np.uint64)
        want1 = np.array([FM.key(g[k], eps, h_field[k]) for k in range(n_max)]).view(np.uint64)
        what = "eps %r sight %r closed %r" % (eps, sight, closed)
        assert np.array_equal(f0[:n_max], want0), what                              # the model knows the plain key
        assert np.array_equal(f1[:n_max], want1), what
        assert np.array_equal(fl1, fl0), what                                       # the flags and the goal test are untouched
        assert np.all(f1[n_max:].view(np.uint8) == POISON) and np.all(fl1[n_max:] == POISON), what
        assert np.array_equal(f2, f0) and np.array_equal(fl2, fl0), what            # clear_field: the plain push again
        assert (want1 != want0).sum() == kinds["G>L"] + kinds["inf"] - int(np.sum((h_field[n_max:n] != h_plain[n_max:n]))), what
        open_bit = 0 if closed else m.search.IS_OPEN
        assert np.all((fl1[:n_max] & m.search.IS_OPEN) == open_bit) and np.all(fl1[:n_max] & m.search.SEEN)
    for b in (fr, opn, tab, fld):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ admissibility
def walls_40():
    """40 x 40 cells of 0.5 m: three walls with gaps at alternating ends between the starts (left) and the goal (right)."""
    c = np.zeros((40, 40), np.int8)  # [y][x]
    c[0:34, 10] = 100
    c[6:40, 20] = 100
    c[0:34, 30] = 100
    return c.ravel()


def test_the_heuristic_is_admissible(engine):
    """64 starts, one goal, ACC controls: the plain search (eps 1, delta 0, no field) gives every found query's optimal
    cost C*; the key a seed is pushed with under the field is its h.  h <= C* (1 + 1e-12), and no found query has h = inf."""
    m = engine
    dims, res = [40, 40], 0.5
    cells = walls_40()
    W, VMAX = 10.0, 1.0
    env = map_env(m, dims, cells, res=res, v_max=VMAX)
    F = env.n_fields
    rng = np.random.default_rng(2024)
    goal = np.zeros(F)
    goal[:2] = [17.75, 2.25]
    free = np.nonzero(cells.reshape(40, 40) == 0)
    starts = np.zeros((F, 64))
    k = 0
    while k < 64:
        j = int(rng.integers(free[0].size))
        y, x = int(free[0][j]), int(free[1][j])
        if k < 40 and x >= 20:
            continue  # most starts two or three walls away from the goal
        starts[:2, k] = [(x + 0.5) * res, (y + 0.5) * res]
        if k % 2:
            starts[2:4, k] = rng.choice([-1.0, 0.0, 1.0], size=2)
        k += 1
    Q = 64
    goals = np.repeat(goal.reshape(1, -1), Q, axis=0)
    lo, hi = FM.goal_box(goal[:2], 0.5, [0.0, 0.0], res)
    want = FM.field(FM.blocked_of(cells), dims, [lo], [hi])
    GL = [FM.heuristic(starts[:2, q], goal, W, VMAX, want[0], dims, [0.0, 0.0], res) for q in range(Q)]
    behind = sum(1 for h, G, L in GL if G is not None and G > L)
    assert behind >= Q / 4 and np.any(starts[2:4] != 0)
    plain = env.search_many(starts, goals, eps=1.0, delta=0.0, capacity=1 << 20, max_frontier=1 << 14, sight=False)
    c_star = np.array(plain.cost)
    found = np.array(plain.found)
    print("found %d of %d, G > L for %d, rounds %d, nodes %d" % (found.sum(), Q, behind, plain.total_rounds, plain.table.stats()[0]))
    plain.free()
    assert found.sum() >= Q / 2
    fld = env.alloc_field().build(goal, 0.5)
    assert np.array_equal(fld.dist(), want)
    tab = env.alloc_table(256, n_queries=Q)
    opn = env.alloc_open(tab)
    opn.set_goals(goals, tol_pos=0.5)
    opn.set_field(fld, np.zeros(Q, np.int32))
    fr = m.TableFrontier(env, Q)
    assert tab.seed(starts, frontier=fr, query=np.arange(Q, dtype=np.int32)) == Q
    opn.push(fr, n_max=Q, eps=1.0)
    env.synchronize()
    h = opn.download()["f"]
    assert np.array_equal(bits(h), bits([x[0] for x in GL]))
    slack = c_star[found] - h[found]
    print("smallest C* - h: %r; largest h / C*: %r" % (slack.min(), np.max(h[found] / c_star[found])))
    assert not np.any(np.isinf(h[found]))
    assert np.all(h[found] <= c_star[found] * (1 + 1e-12))
    for b in (fr, opn, tab, fld):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------------ the search
def trap_cells(gap=False):
    """61 x 61 cells: a U-shaped wall three cells thick, open towards low y; gap: three cells of its closed end are free."""
    c = np.zeros((61, 61), np.int8)  # [y][x]
    c[15:46, 18:21] = 100
    c[15:46, 40:43] = 100
    c[43:46, 18:43] = 100
    if gap:
        c[43:46, 29:32] = 0
    return c.ravel()


def trap_env(m, gap=False):
    env = map_env(m, [61, 61], trap_cells(gap), res=0.5)
    start = m.Waypoint(2, m.ACC, pos=[15.25, 17.75]).to_row()   # inside the cup
    goal = m.Waypoint(2, m.ACC, pos=[15.25, 26.25]).to_row()    # behind its closed end
    return env, start, goal


KW = dict(eps=1.0, delta=0.0, capacity=1 << 17, max_frontier=1 << 13)


def test_search_corridor_with_a_field(engine):
    from test_gpu_open import corridor_env
    m = engine
    env, start, goal = corridor_env(m)
    r = env.search(start, goal, eps=1.0, delta=0.0, capacity=1 << 15, max_frontier=4096, field=True)
    print("corridor with a field:", r, "field passes", r.field.passes)
    assert r.status == m.search.FOUND and r.cost == 351.5 and r.field.F == 1
    r.free()
    env.close()


def test_search_trap(engine):
    """The test that cannot pass without the field: the start inside a cup, the goal behind its closed end.  Recorded on an
    MI355X: see DESIGN.md 4.21."""
    m = engine
    env, start, goal = trap_env(m)
    plain = env.search(start, goal, **KW)
    with_field = env.search(start, goal, field=True, **KW)
    print("trap plain:", plain, plain.table.stats())
    print("trap field:", with_field, with_field.table.stats(), "passes", with_field.field.passes)
    assert plain.status == m.search.FOUND and with_field.status == m.search.FOUND
    assert with_field.cost == plain.cost and with_field.last_select["goal_g"] == plain.last_select["goal_g"]
    assert with_field.expanded < plain.expanded
    fld = with_field.field
    assert fld.F == 1 and with_field._owns_field
    with_field.free()
    assert fld._fld is None  # freed with the result
    plain.free()
    env.close()


def test_search_many_shares_one_field(engine):
    """Eight delay-style queries on one goal among a reservation: one field, and every query equals its own search(field=True)."""
    m = engine
    env, start, goal = trap_env(m)
    other = m.Waypoint(2, m.ACC, pos=[12.25, 17.75]).to_row()
    solo = env.search(other, goal, **KW)
    p = solo.path()
    res = env.alloc_reservations((p[0].reshape(-1, 1), p[1].reshape(-1, 1)), 0.25, n_steps=400, radius=0.4)
    delays = 0.5 * np.arange(8)
    kw = dict(KW, capacity=1 << 19, avoid=res, radius=0.4)
    many = env.search_many(np.repeat(start.reshape(-1, 1), 8, axis=1), np.repeat(goal.reshape(1, -1), 8, axis=0), t0=delays, field=True, **kw)
    assert many.field.F == 1 and many._field_of_query.tolist() == [0] * 8
    print("many:", many)
    for q in range(8):
        one = env.search(start, goal, t0=float(delays[q]), field=True, **dict(kw, capacity=1 << 17))
        a = (one.status, one.cost, one.rounds, one.expanded, one.path()[1].tolist() if one.found else None)
        b = (many.status[q], many.cost[q], many.rounds[q], many.expanded[q], many.path(q)[1].tolist() if many.found[q] else None)
        assert a == b, (q, a, b)
        one.free()
    assert any(many.found)
    for x in (many, res, solo):
        x.free()
    env.close()


def test_plan_prioritised_with_fields(engine):
    from test_gpu_wait import STEP, lane_env
    m = engine
    n = 33
    cells = np.full((n, n), 100, np.int8)
    cells[16, :] = 0
    cells[:, 16] = 0
    env = lane_env(m, cells)
    wp = lambda p: m.Waypoint(2, m.ACC, pos=p).to_row()
    starts = np.stack([wp([2.5, 16.5]), wp([16.5, 12.5])], axis=1)
    goals = np.stack([wp([30.5, 16.5]), wp([16.5, 16.5])])
    kw = dict(capacity=1 << 17, max_frontier=4096, n_steps=int(120 / STEP), eps=1.0, delta=0.0, wait=True, park_goal=True)
    a = m.search.plan_prioritised(env, starts, goals, STEP, 0.3, field=False, **kw)
    b = m.search.plan_prioritised(env, starts, goals, STEP, 0.3, field=True, **kw)
    print("prioritised:", a["status"], a["cost"], b["status"], b["cost"])
    assert b["status"] == [m.search.FOUND] * 2 and not b["conflicts"].charged.any()
    assert list(b["cost"]) == list(a["cost"])
    env.close()


def test_search_across_cost_cells_of_a_potential_map(engine):
    """A potential map whose cost cells (30) lie across every route and whose blocking cells (100) make a wall with a gap:
    cost cells are traversable for the field as they are for a primitive.  With and without the field the search is FOUND
    at equal cost, and the start's h is not above it -- from left of the band, from a cost cell, from the right."""
    m = engine
    dims, res = [40, 30], 0.5
    pot = np.zeros((30, 40), np.int8)  # [y][x]
    pot[:, 12:15] = 30                 # a band of cost cells from edge to edge
    pot[0:24, 24] = 100                # a blocking wall, its gap at high y
    pot[24:30, 24] = 5
    pot = pot.ravel()
    env = map_env(m, dims, np.zeros(40 * 30, np.int8), res=res)
    env.set_potential_map(pot)
    F = env.n_fields
    goal = np.zeros(F)
    goal[:2] = [17.25, 2.25]
    lo, hi = FM.goal_box(goal[:2], 0.5, [0.0, 0.0], res)
    want = FM.field(pot >= 100, dims, [lo], [hi])
    fld = env.alloc_field().build(goal, 0.5)
    assert np.array_equal(fld.dist(), want)
    kw = dict(eps=1.0, delta=0.0, capacity=1 << 17, max_frontier=1 << 13, sight=False)
    behind = 0
    for pos in ([2.25, 2.25], [6.75, 7.25], [9.25, 2.25]):
        start = np.zeros(F)
        start[:2] = pos
        h, G, L = FM.heuristic(pos, goal, float(env._p.w), 1.0, want[0], dims, [0.0, 0.0], res)
        plain = env.search(start, goal, **kw)
        with_field = env.search(start, goal, field=fld, **kw)
        print("potential", pos, "h", h, "G", G, "L", L, plain, with_field)
        assert plain.status == m.search.FOUND and with_field.status == m.search.FOUND
        assert with_field.cost == plain.cost and np.isfinite(h) and h <= plain.cost * (1 + 1e-12)
        assert with_field.expanded <= plain.expanded
        behind += G > L
        plain.free()
        with_field.free()
    assert behind == 3 and pot[FM.cell_of([6.75, 7.25], dims, [0.0, 0.0], res)] == 30
    fld.free()
    env.close()


def test_replan_rebuilds_an_owned_field(engine):
    m = engine
    env, start, goal = trap_env(m)
    r0 = env.search(start, goal, field=True, **KW)
    fld = r0.field
    assert r0.found and not fld.stale
    new = trap_cells(gap=True)
    changed = np.nonzero(new != trap_cells())[0]
    env.editMap(changed, new[changed])
    assert fld.stale
    r1 = r0.replan()
    assert r0.table is None and r0.field is None and r1.field is fld and r1._owns_field and not fld.stale
    lo, hi = FM.goal_box(goal[:2], 0.5, [0.0, 0.0], 0.5)
    assert np.array_equal(fld.dist(), FM.field(FM.blocked_of(new), [61, 61], [lo], [hi]))
    fresh = env.search(start, goal, field=True, **KW)
    print("replan:", r0.cost, "->", r1, "fresh:", fresh)
    assert r1.found and fresh.found and r1.cost == fresh.cost and r1.cost < r0.cost
    # a caller's field that went stale is refused
    mine = env.alloc_field().build(goal, 0.5)
    r2 = env.search(start, goal, field=mine, **KW)
    assert r2.found and r2.cost == fresh.cost and r2.field is mine and not r2._owns_field
    env.editMap(changed[:1], [100])
    with pytest.raises(RuntimeError):
        r2.replan()
    r2.free()
    assert mine._fld is not None  # not freed with the result
    for x in (mine, fresh, r1):
        x.free()
    env.close()


def test_without_a_field_nothing_changed(engine):
    """field=None: what the parent commit returns (the two builds, run side by side on an MI355X, printed the same
    lines): status, cost, rounds, expansions, node counts and path."""
    from test_gpu_open import corridor_env
    from test_multi import corridor_queries
    m = engine
    env, start, goal = corridor_env(m)
    starts, goals = corridor_queries(m)
    one = env.search(start, goal, capacity=1 << 15, max_frontier=4096)
    many = env.search_many(starts[:, :3], goals[:3], capacity=1 << 17, max_frontier=4096)
    got = (one.status, one.cost, one.rounds, one.expanded, one.table.stats(), one.path()[1].tolist())
    got_many = (many.status, many.cost, many.rounds, many.expanded, many.total_rounds, many.table.stats(),
                [many.path(q)[1].tolist() for q in range(3)])
    print("UNCHANGED one:", got)
    print("UNCHANGED many:", got_many)
    assert one.field is None and many.field is None
    assert got == PARENT_ONE
    assert got_many == PARENT_MANY
    zero = env.search(start, goal, eps=1.0, delta=0.0, capacity=1 << 15, max_frontier=4096)
    got_zero = (zero.status, zero.cost, zero.rounds, zero.expanded, zero.table.stats(), zero.path()[1].tolist())
    print("UNCHANGED delta 0:", got_zero)
    assert got_zero == PARENT_ZERO
    for x in (one, many, zero):
        x.free()
    env.close()


# printed by the parent build and by this one, run side by side on an MI355X
PATHS = [[7, 7, 4, 5, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4], [7, 7, 4, 4, 5, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 3, 4], [1, 1, 4, 3, 4, 4, 5, 4, 4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 5, 4]]
PARENT_ONE = (1, 351.5, 35, 6073, (10102, 0), PATHS[0])
PARENT_MANY = ([1, 1, 1], [351.5, 351.75, 352.0], [35, 35, 35], [6073, 6117, 5949], 35, (30239, 0), PATHS)
PARENT_ZERO = (1, 351.5, 49, 586, (1780, 0), [7, 7, 4, 5, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 5, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4])
