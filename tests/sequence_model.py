"""Host-side model of what a long-lived context should hold, the alphabet of operations that change it, and the
generator of the operation sequences of tests/test_gpu_sequences.py.  Pure numpy + the CPU oracle: nothing here touches
the engine, so the plans (and whether each step of them can be noticed at all) are checked on a machine without a GPU.

The model holds what the reference's env_map + MapUtil would: map cells, geometry, potential map, search region, control
flag, control table, the parameters of mplx_params and the goal.  Every operation updates it with a restatement the
suite already pins to the reference: np_dilate / np_free_unknown (tests/test_map_util.py), oracle.update_potential_map
/ oracle.search_region (tests/test_map_prep.py), plain indexing for editMap (a cell named twice takes its last value).
Where the reference has no rule the context's documented one is restated: a setMap with another geometry drops the
potential map and the region; with a potential map installed the blocked test reads THAT map (env_map.h:113-118), so
an edit of the occupancy shows in the lists only once the potential map is removed."""
import copy
import functools

import numpy as np

from oracle import oracle as O
from test_gpu_parity import _small_world
from test_map_util import ball, box, np_dilate, np_free_unknown

N_SMALL = 24       # the host-pointer batch (what the resident service kernel serves) = the probe of the discrimination tests
N_RES = 192        # the resident launch below the 4096 nodes that rebuild the free-box table
N_DISTINCT = 512   # distinct probe nodes; the launch of >= 4096 nodes repeats them
N_BIG = 4096
FULL_ROWS_MAX_NU = 64  # the 4096-node launch asks for every row up to this table size, count/action/cost/hash above it

PARAM_KEYS = ("dt", "w", "wyaw", "v_max", "a_max", "j_max", "yaw_max", "potential_weight", "gradient_weight")

# slice -> (dimension, control flag, map axis lengths (cells % 32 != 0: the map ends in a partial word), seed)
SLICES = {
    "2d_acc": dict(dim=2, control=0x03, dims=[47, 45], seed=9100),
    "3d_acc": dict(dim=3, control=0x03, dims=[45, 43, 41], seed=9200),
    "2d_yaw_pot": dict(dim=2, control=0x13, dims=[47, 45], seed=9300),
}

MUTATORS = ("setmap_same", "setmap_size", "setmap_origin", "setmap_res", "edit", "dilate", "free_unknown",
            "pot_set", "p_potw", "p_yaw", "pot_off", "pot_update", "free_all", "region_set", "region_off", "region_path",
            "p_limits", "p_time", "p_cost", "control", "u_table", "goal_set", "goal_clear")
NEUTRALS = ("route", "service", "read_cells", "clouds", "check_edges", "post_lists", "pack_lists", "synchronize",
            "map_upload_bytes")
# kinds whose effect exists only with a yaw flag / an installed potential map
YAW_ONLY = ("p_yaw",)
NEED_POTENTIAL = ("pot_off", "p_potw")
YAW_SLICE_KINDS = ("p_yaw", "p_potw", "pot_set", "pot_off", "pot_update")
# operations on the occupancy map: hidden behind an installed potential map
OCCUPANCY_OPS = ("setmap_same", "edit", "dilate", "free_unknown", "free_all")


class Model:
    def __init__(self, dim, control, U, cells, map_dim, origin, res, params, potential=None, region=None, goal=None):
        self.dim, self.control = int(dim), int(control)
        self.U = np.ascontiguousarray(U, dtype=np.float64)
        self.cells = np.array(cells, dtype=np.int8).ravel()
        self.map_dim = [int(x) for x in map_dim]
        self.origin = [float(x) for x in origin]
        self.res = float(res)
        self.params = dict(params)
        self.potential = None if potential is None else np.array(potential, dtype=np.int8).ravel()
        self.region = None if region is None else np.array(region, dtype=np.uint8).ravel()
        self.goal = goal  # dict(row, control, w, v_max, tol_pos, tol_vel, tol_acc, tol_yaw) or None

    def copy(self):
        return copy.deepcopy(self)

    @property
    def nU(self):
        return self.U.shape[0]

    @property
    def n_cells(self):
        return int(np.prod(self.map_dim))

    def shaped(self):
        return self.cells.reshape(tuple(reversed(self.map_dim)))

    def oracle_env(self, without_potential=False):
        return O.Env(self.dim, self.control, self.U, self.cells, self.map_dim, self.origin, self.res,
                     potential=None if without_potential else self.potential, region=self.region, **self.params)

    def service_eligible(self):
        """plan_tile (lists_route.cpp) restated for the tables of this module: the configurations the resident kernel serves."""
        p = self.params
        if self.control & 0x10 or self.potential is not None or self.nU > 1024:
            return False
        vb = float(np.abs(self.U[:, :self.dim]).max()) if (self.control & 0x0F) == 0x01 else p["v_max"]
        return vb > 0 and np.ceil(vb * p["dt"] / self.res) + 1.0 <= 63.0


class Op:
    """One operation: `call` is what the driver sends to EnvMap (name + arguments), `kind` its entry of the alphabet."""

    def __init__(self, kind, call, label):
        self.kind, self.call, self.label = kind, call, label

    def __repr__(self):
        return "%s[%s]" % (self.kind, self.label)


def apply_to_model(m, op):
    """The model after `op` (in place).  Neutral operations change nothing."""
    c = op.call
    name = c[0]
    if name == "setMap":
        _, origin, dims, cells, res = c
        same = list(dims) == m.map_dim and list(origin) == m.origin and float(res) == m.res
        if not same:
            m.potential = None
            m.region = None
        m.cells = np.array(cells, dtype=np.int8).ravel()
        m.map_dim, m.origin, m.res = [int(x) for x in dims], [float(x) for x in origin], float(res)
    elif name == "editMap":
        for i, v in zip(c[1], c[2]):  # in order: the last mention of a cell wins
            m.cells[int(i)] = v
    elif name == "dilate":
        m.cells = np_dilate(m.cells, m.map_dim, c[1]).astype(np.int8)
    elif name == "freeUnknown":
        m.cells = np_free_unknown(m.cells)
    elif name == "freeAll":
        m.cells = np.zeros_like(m.cells)
    elif name == "set_potential_map":
        m.potential = None if c[1] is None else np.array(c[1], dtype=np.int8).ravel()
    elif name == "updatePotentialMap":
        _, pos, radius, range_, power = c
        # the reference replaces the map by the potential-valued map and installs it as the potential map
        new = O.update_potential_map(m.cells, m.map_dim, m.origin, m.res, pos, radius, range_, power)
        m.cells = new.copy()
        m.potential = new.copy()
    elif name == "set_search_region":
        m.region = None if c[1] is None else (np.asarray(c[1]) != 0).astype(np.uint8).ravel()
    elif name == "setSearchRegion":
        _, path, radius, dense = c
        m.region = O.search_region(m.map_dim, m.origin, m.res, path, radius, dense)
    elif name == "set_param":
        m.params[c[1]] = float(c[2])
    elif name == "set_control":
        m.control = int(c[1])
    elif name == "set_u":
        m.U = np.ascontiguousarray(c[1], dtype=np.float64)
    elif name == "set_goal":
        m.goal = None if c[1] is None else dict(c[1], control=m.control)  # hashed with the flag in force at the call
    elif name in NEUTRALS:
        pass
    else:
        raise ValueError(name)
    return m


# ------------------------------------------------------------------------------------------------------------- worlds
def _sprinkle_unknown(cells, seed):
    """~6 % of the free cells become unknown (-1): MapUtil::freeUnknown and the unknown cloud have something to do."""
    out = np.array(cells, dtype=np.int8).ravel().copy()
    rng = np.random.default_rng(seed)
    free = np.nonzero(out == 0)[0]
    out[rng.choice(free, free.size // 16, replace=False)] = -1
    return out


def make_cells(dims, res, seed):
    import motion_primitive_library_amd.workloads as W
    return _sprinkle_unknown(W.box_map(dims, res, 0.15, seed, side_m=(0.3, 1.2)), seed + 5)


def _tables(dim, yaw):
    import motion_primitive_library_amd.workloads as W
    g = W.grid_controls
    rng = np.random.default_rng(41 + dim)
    lin = lambda n: list(np.round(np.linspace(-1.0, 1.0, n), 4))
    if yaw:
        rates = [-0.5, 0.0, 0.5]
        base = g([-1.0, 0.0, 1.0], dim, yaw_rates=rates)
        return [("base27", base), ("two_rates18", g([-1.0, 0.0, 1.0], dim, yaw_rates=[-0.5, 0.5])),
                ("shuffled27", base[rng.permutation(base.shape[0])]),
                ("ten_by_three30", np.array([[a, b, y] for a in lin(5) for b in (-0.5, 0.5) for y in rates]))]
    if dim == 2:
        base = g([-1.0, -0.5, 0.0, 0.5, 1.0], 2)
        return [("base25", base), ("nine", g([-1.0, 0.0, 1.0], 2)), ("shuffled25", base[rng.permutation(25)]),
                ("wide34", np.array([[a, b] for a in lin(17) for b in (-0.5, 0.5)])),          # 17 values on an axis
                ("yaw_column75", g([-1.0, -0.5, 0.0, 0.5, 1.0], 2, yaw_rates=[-0.5, 0.0, 0.5])),  # unused under ACC
                ("wide272", np.array([[a, b] for a in lin(17) for b in lin(16)])),             # >= 256: line padding
                ("huge1056", np.array([[a, b] for a in lin(33) for b in lin(32)]))]            # > 1024: no tile kernel
    base = g([-1.0, 0.0, 1.0], 3)
    return [("base27", base), ("eighteen", np.array([[a, b, c] for a in lin(3) for b in lin(3) for c in (-0.5, 0.5)])),
            ("shuffled27", base[rng.permutation(27)]),
            ("wide34", np.array([[a, b, 0.5] for a in lin(17) for b in (-0.5, 0.5)])),
            ("yaw_column54", np.array([[a, b, c, y] for a in lin(3) for b in lin(3) for c in lin(3) for y in (-0.5, 0.5)])),
            ("wide272", np.array([[a, b, c] for a in lin(17) for b in lin(4) for c in lin(4)])),
            ("huge1100", np.array([[a, b, c] for a in lin(11) for b in lin(10) for c in lin(10)]))]


class World:
    """What a slice's plans are drawn from: the base model, the probe frontier and the variants of every kind."""

    def __init__(self, name):
        import motion_primitive_library_amd as pkg
        s = SLICES[name]
        self.name, self.dim, self.control, self.seed = name, s["dim"], s["control"], s["seed"]
        self.yaw = bool(self.control & 0x10)
        dim = self.dim
        wl = _small_world(pkg, dim, 0x1F, seed=s["seed"], n_nodes=N_DISTINCT, region=True, dims=s["dims"])
        nodes = np.roll(wl.nodes, -4 * dim, axis=1)  # (the nodes pinned to the map borders go last, not into the small batch)
        if self.yaw:  # headings near the direction of travel: the heading limit leaves most primitives valid
            rng = np.random.default_rng(s["seed"] + 3)
            nodes[4 * dim] = np.arctan2(nodes[dim + 1], nodes[dim]) + rng.uniform(-0.3, 0.3, size=N_DISTINCT)
        else:
            nodes[4 * dim] = 0.0
        self.probes = np.ascontiguousarray(nodes)
        self.tables = _tables(dim, self.yaw)
        params = {"dt": 1.0, "w": 10.0, "wyaw": 1.0, "v_max": 1.5, "a_max": 1.0, "j_max": 1.5,
                  "yaw_max": 0.6 if self.yaw else -1.0, "potential_weight": 0.1, "gradient_weight": 0.0}
        import motion_primitive_library_amd.workloads as W
        ext = [d * 0.1 for d in s["dims"]]
        region = W.tunnel_region(s["dims"], [0.0] * dim, 0.1, [0.5] * dim, [e - 0.5 for e in ext], 1.0 if dim == 2 else 1.6)
        self.base = Model(dim, self.control, self.tables[0][1], _sprinkle_unknown(wl.grid, s["seed"] + 5), s["dims"],
                          [0.0] * dim, 0.1, params, region=region)
        self.size_alts = [[40, 52], [47, 45], [53, 38]] if dim == 2 else [[40, 47, 38], [45, 43, 41], [36, 50, 44]]
        self.origin_alts = [[0.0] * dim, [0.05, -0.1, 0.15][:dim], [-0.2, 0.1, -0.05][:dim]]
        self.res_alts = [0.1, 0.125, 0.08]
        self.controls = [0x11, 0x17, 0x13] if self.yaw else [0x07, 0x01, 0x0F, 0x03]

    @property
    def small(self):
        return np.ascontiguousarray(self.probes[:, :N_SMALL])

    def warm(self, potential=False, goal=True):
        m = self.base.copy()
        if goal:
            apply_to_model(m, _goal_ops(self, m)[0])
        if potential:
            apply_to_model(m, _pot_set_ops(self, m)[0])
            m.params["potential_weight"] = 0.1
        return m


@functools.lru_cache(maxsize=None)
def world(name):
    return World(name)


# ----------------------------------------------------------------------------------------- what a step can be seen by
def probe_lists(m, nodes, without_potential=False):
    r = O.expand(m.oracle_env(without_potential), nodes, threads=2)
    return r


def _lists_differ(a, b):
    if a["status"].shape != b["status"].shape:
        return True
    if not np.array_equal(a["status"], b["status"]):
        return True
    emit = (a["status"] == 1) | (a["status"] == 2)
    return not (np.array_equal(a["cost"][emit].view(np.uint64), b["cost"][emit].view(np.uint64))
                and np.array_equal(a["hash"][emit], b["hash"][emit]) and np.array_equal(a["iters"][emit], b["iters"][emit])
                and np.array_equal(a["state"][:, emit].view(np.uint64), b["state"][:, emit].view(np.uint64)))


def fused_rows(m, ref):
    """heur / flags of the emitted successors of `ref` under the model's goal (env_base.h:46-64, env_map.h:25-37)."""
    g, D = m.goal, m.dim
    emit = (ref["status"] == 1) | (ref["status"] == 2)
    st = ref["state"][:, emit]
    goal = np.asarray(g["row"], dtype=np.float64)
    linf = lambda lo: np.abs(st[lo:lo + D] - goal[lo:lo + D, None]).max(axis=0)
    same = ref["hash"][emit] == np.uint64(O.lattice_hash(D, g["control"], goal))
    heur = np.where(same, 0.0, g["w"] * linf(0) / g["v_max"] if g["v_max"] > 0 else g["w"] * linf(0))
    ok = linf(0) <= g["tol_pos"]
    if g["tol_vel"] >= 0:
        ok &= linf(D) <= g["tol_vel"]
    if g["tol_acc"] >= 0:
        ok &= linf(2 * D) <= g["tol_acc"]
    if g["tol_yaw"] >= 0:
        ok &= np.abs(st[4 * D] - goal[4 * D]) <= g["tol_yaw"]
    return heur, ok.astype(np.uint8) | (same.astype(np.uint8) << 1)


def effect(before, after, op, nodes):
    """How the step shows on the probe frontier `nodes`, oracle alone:
    "lists"  the successor lists differ,
    "fused"  the lists are the same, the heur / flags rows (or whether a launch may ask for them) differ,
    "hidden" an operation on the occupancy behind an installed potential map: the lists are EQUAL, as the rule demands,
             and differ once the potential map is taken away,
    "cells"  the lists are the same and the map cells differ (read_cells / the clouds see it),
    None     nothing an observer could notice."""
    a, b = probe_lists(before, nodes), probe_lists(after, nodes)
    if _lists_differ(a, b):
        return "lists"
    if (before.goal is None) != (after.goal is None):
        return "fused"
    if after.goal is not None:
        fa, fb = fused_rows(before, a), fused_rows(after, b)
        if not (np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])):
            return "fused"
    if before.potential is not None and after.potential is not None and op.kind in OCCUPANCY_OPS:
        if _lists_differ(probe_lists(before, nodes, True), probe_lists(after, nodes, True)):
            return "hidden"
    if before.cells.shape != after.cells.shape or not np.array_equal(before.cells, after.cells):
        return "cells"
    return None


def structural_reason(before, kind):
    """Why a step of `kind` applied to the model `before` cannot change a successor list, whatever its arguments."""
    if kind == "free_unknown":
        return "the expansion blocks on cells == 100 alone (map_util.h:48): unknown cells are free to it; read_cells and the clouds see the step"
    if kind in ("pot_off", "p_potw") and before.potential is None:
        return "no potential map is installed: nothing to remove, nothing the weights multiply"
    if kind == "p_limits" and (before.control & 0x0F) == 0x01:
        return "control flag VEL: the velocity of a primitive is its control, no limit is consulted"
    if kind == "p_yaw" and not before.control & 0x10:
        return "no yaw flag: yaw_max and wyaw are not consulted"
    if kind == "region_off" and before.region is None:
        return "no region is installed"
    if kind == "goal_clear" and before.goal is None:
        return "no goal is set"
    if kind in ("dilate", "free_all", "pot_set", "pot_update") and not np.any(before.cells > 0):
        return "the map has no occupied cell: nothing to dilate, free or derive a potential field from"
    return None


# Steps of the tables that no rule above explains and that still change no list of the 24-node batch, found by running the
# generator: listed so that tests/test_gpu_sequences.py::test_every_step_of_the_tables_can_be_noticed knows them by name.
BY_CHANCE = {
    ("2d_acc", "control>free_all", 1): "under the flag the first step chose no successor of the batch is blocked by an occupied cell "
                                       "(the region and the map border block them); the map read-back sees the step",
    ("3d_acc", "control>free_all", 1): "as in 2D",
}


# ------------------------------------------------------------------------------------------- the variants of a kind
def _end_cells(w, m):
    """Cells in which successors of the small batch end (free ones): blocking them changes those successors."""
    r = probe_lists(m, w.small)
    pos = r["state"][:m.dim, r["status"] == 1]
    pn = np.round((pos - np.asarray(m.origin)[:, None]) / m.res - 0.5).astype(np.int64)
    ok = np.all((pn >= 0) & (pn < np.asarray(m.map_dim)[:, None]), axis=0)
    pn = pn[:, ok]
    idx = pn[0].copy()
    mul = 1
    for i in range(1, m.dim):
        mul *= m.map_dim[i - 1]
        idx += mul * pn[i]
    idx = np.unique(idx)
    idx = idx[m.cells[idx] != 100]
    return idx[::3][:40]


def _edit_ops(w, m):
    T = _end_cells(w, m)
    if T.size == 0:
        T = np.nonzero(m.cells != 100)[0][:8]
    rng = np.random.default_rng(w.seed + m.n_cells)
    occ = np.nonzero(m.cells == 100)[0]
    occ = rng.choice(occ, min(30, occ.size), replace=False) if occ.size else occ
    n = m.n_cells
    words = np.unique(T[:4] // 32)
    shared = np.concatenate([np.arange(32 * wd, min(32 * wd + 32, n)) for wd in words])
    last = np.arange(32 * ((n - 1) // 32), n)
    i8 = lambda v, k: np.full(k, v, np.int8)
    return [
        Op("edit", ("editMap", T.copy(), i8(100, T.size)), "sorted_unique"),
        Op("edit", ("editMap", np.concatenate([T, occ, T[::-1], occ]),
                    np.concatenate([i8(0, T.size), i8(100, occ.size), i8(100, T.size), i8(0, occ.size)])), "duplicates"),
        Op("edit", ("editMap", np.concatenate([shared[::-1], T]),
                    np.concatenate([np.where(shared[::-1] % 2 == 0, 100, 0).astype(np.int8), i8(100, T.size)])), "shared_word"),
        Op("edit", ("editMap", np.concatenate([T, last]), np.concatenate([i8(100, T.size), i8(100, last.size)])), "last_word"),
    ]


def _dilate_ops(w, m):
    dim = m.dim
    axes = np.concatenate([np.eye(dim, dtype=np.int32), -np.eye(dim, dtype=np.int32)])
    asym = np.array([[1, 0, 0], [2, 0, 0], [0, -3, 1], [-1, 2, 0], [0, 0, 0], [3, -1, 1]], dtype=np.int32)[:, :dim]
    return [Op("dilate", ("dilate", o), n) for n, o in (("axes", axes), ("box", box(dim)), ("asymmetric", asym), ("ball2", ball(2, dim)))]


def _pot_set_ops(w, m):
    import motion_primitive_library_amd.workloads as W
    out = []
    for r in (0.4, 0.3, 0.5):
        pot = W.potential_field(m.shaped(), m.res, r, r if m.dim == 3 else None)
        out.append(Op("pot_set", ("set_potential_map", pot.ravel()), "radius%.1f" % r))
    return out


def _pot_update_ops(w, m):
    centre = [m.origin[i] + m.map_dim[i] * m.res * 0.5 for i in range(m.dim)]
    v = lambda a, b: ([a, a, b][:m.dim] if m.dim == 3 else [a, a])
    return [Op("pot_update", ("updatePotentialMap", centre, v(0.4, 0.4), None, 1.0), "global"),
            Op("pot_update", ("updatePotentialMap", centre, v(0.3, 0.2), v(1.5, 1.5), 1.0), "range_box"),
            Op("pot_update", ("updatePotentialMap", centre, v(0.5, 0.3), None, 2.0), "power2"),
            Op("pot_update", ("updatePotentialMap", centre, v(0.35, 0.35), v(1.0, 0.8), 0.5), "range_box_sqrt")]


def _extent(m):
    return [m.map_dim[i] * m.res for i in range(m.dim)]


def _region_set_ops(w, m):
    import motion_primitive_library_amd.workloads as W
    e, o, D = _extent(m), m.origin, m.dim
    lo = [o[i] + 0.5 for i in range(D)]
    hi = [o[i] + e[i] - 0.5 for i in range(D)]
    anti0, anti1 = [hi[0]] + lo[1:], [lo[0]] + hi[1:]
    mid = [o[i] + 0.5 * e[i] for i in range(D)]
    band0, band1 = [lo[0]] + mid[1:], [hi[0]] + mid[1:]
    return [Op("region_set", ("set_search_region", W.tunnel_region(m.map_dim, o, m.res, p0, p1, r).ravel()), n)
            for n, p0, p1, r in (("diagonal", lo, hi, 0.6 * D - 0.2), ("antidiagonal", anti0, anti1, 0.5 * D), ("band", band0, band1, 0.45 * D))]


def _region_path_ops(w, m):
    e, o, D = _extent(m), m.origin, m.dim
    f = lambda *t: [o[i] + t[i] * e[i] for i in range(D)]
    zig = np.array([f(0.1, 0.2, 0.3), f(0.5, 0.8, 0.6), f(0.9, 0.3, 0.4)])
    out_of_map = np.array([f(0.2, 0.7, 0.5), f(0.6, 0.4, 0.5), f(1.2, 1.1, 0.9)])  # ends outside the map
    return [Op("region_path", ("setSearchRegion", zig, [0.3 * D] * D, False), "zigzag"),
            Op("region_path", ("setSearchRegion", out_of_map, [0.9, 0.7, 1.1][:D], False), "leaves_the_map"),
            Op("region_path", ("setSearchRegion", zig, [0.5 * D] * D, True), "points_only")]


def _goal_ops(w, m):
    e, o, D = _extent(m), m.origin, m.dim
    out = []
    for k, (frac, w_h, v_h, tp, tv) in enumerate(((0.7, 10.0, 1.5, 0.5, -1.0), (0.3, 3.0, 1.0, 0.8, 1.0), (0.5, 10.0, -1.0, 1.2, -1.0))):
        row = np.zeros(4 * D + 2)
        row[:D] = [o[i] + frac * e[i] for i in range(D)]
        out.append(Op("goal_set", ("set_goal", dict(row=row, w=w_h, v_max=v_h, tol_pos=tp, tol_vel=tv, tol_acc=-1.0, tol_yaw=-1.0)),
                      "goal%d" % k))
    return out


def _param_ops(kind, pairs):
    return [Op(kind, ("set_param", n, v), "%s=%g" % (n, v)) for n, v in pairs]


def variants(w, m, kind):
    D = m.dim
    if kind == "setmap_same":
        return [Op(kind, ("setMap", m.origin, m.map_dim, make_cells(m.map_dim, m.res, w.seed + 11 * k), m.res), "cells%d" % k)
                for k in (1, 2, 3)]
    if kind == "setmap_size":
        return [Op(kind, ("setMap", m.origin, d, make_cells(d, m.res, w.seed + 50 + k), m.res), "x".join(map(str, d)))
                for k, d in enumerate(w.size_alts) if d != m.map_dim]
    if kind == "setmap_origin":
        return [Op(kind, ("setMap", o, m.map_dim, m.cells.copy(), m.res), "origin%d" % k)
                for k, o in enumerate(w.origin_alts) if o != m.origin]
    if kind == "setmap_res":
        return [Op(kind, ("setMap", m.origin, m.map_dim, m.cells.copy(), r), "res%g" % r) for r in w.res_alts if r != m.res]
    if kind == "edit":
        return _edit_ops(w, m)
    if kind == "dilate":
        return _dilate_ops(w, m)
    if kind == "free_unknown":
        return [Op(kind, ("freeUnknown",), "")]
    if kind == "free_all":
        return [Op(kind, ("freeAll",), "")]
    if kind == "pot_set":
        return _pot_set_ops(w, m)
    if kind == "pot_off":
        return [Op(kind, ("set_potential_map", None), "")]
    if kind == "pot_update":
        return _pot_update_ops(w, m)
    if kind == "region_set":
        return _region_set_ops(w, m)
    if kind == "region_off":
        return [Op(kind, ("set_search_region", None), "")]
    if kind == "region_path":
        return _region_path_ops(w, m)
    if kind == "p_limits":
        if (m.control & 0x0F) == 0x01:  # VEL: the velocity of a primitive is its control; no other limit is consulted
            return _param_ops(kind, [("v_max", v) for v in (0.7, -1.0, 1.5) if v != m.params["v_max"]])
        return _param_ops(kind, [("v_max", 1.0), ("a_max", 0.6), ("v_max", -1.0), ("j_max", 0.8), ("a_max", -1.0), ("j_max", -1.0),
                                 ("v_max", 1.5), ("a_max", 1.0), ("j_max", 1.5)])
    if kind == "p_time":
        return _param_ops(kind, [("dt", v) for v in (0.8, 1.25, 1.0) if v != m.params["dt"]])
    if kind == "p_cost":
        return _param_ops(kind, [("w", v) for v in (3.5, 12.25, 10.0) if v != m.params["w"]])
    if kind == "p_yaw":
        return _param_ops(kind, [("yaw_max", 0.4), ("wyaw", 0.0), ("yaw_max", -1.0), ("wyaw", 0.8), ("yaw_max", 0.6), ("wyaw", 1.0)])
    if kind == "p_potw":
        return _param_ops(kind, [("potential_weight", 0.5), ("gradient_weight", 0.25), ("potential_weight", 0.1), ("gradient_weight", 0.0)])
    if kind == "control":
        return [Op(kind, ("set_control", c), "0x%02x" % c) for c in w.controls if c != m.control]
    if kind == "u_table":
        return [Op(kind, ("set_u", U), n) for n, U in w.tables if U.shape != m.U.shape or not np.array_equal(U, m.U)]
    if kind == "goal_set":
        return _goal_ops(w, m)
    if kind == "goal_clear":
        return [Op(kind, ("set_goal", None), "")]
    raise ValueError(kind)


def make_step(w, m, kind, rot):
    """The variant of `kind` the rotation `rot` points at -- or the next one that can be noticed on the small batch, if
    that one cannot (e.g. j_max under ACC).  Applies it to the model; returns (op, effect)."""
    cand = variants(w, m, kind)
    first = None
    for k in range(len(cand)):
        op = cand[(rot + k) % len(cand)]
        after = apply_to_model(m.copy(), op)
        eff = effect(m, after, op, w.small)
        if first is None:
            first = (op, after, eff)
        if eff in ("lists", "fused", "hidden"):
            first = (op, after, eff)
            break
    op, after, eff = first
    m.__dict__.update(after.__dict__)
    return op, eff


# ------------------------------------------------------------------------------------------------------------- plans
class Plan:
    """warm: the model the fresh context is configured to; steps: [(op, model after it, effect or None for neutral ops)]."""

    def __init__(self, slice_name, warm, steps, label):
        self.slice, self.warm, self.steps, self.label = slice_name, warm, steps, label

    def models(self):
        return [self.warm] + [s[1] for s in self.steps]

    def describe(self, upto=None):
        return "%s %s: %s" % (self.slice, self.label, " -> ".join(repr(s[0]) for s in self.steps[:upto]))


def pair_kinds(slice_name):
    """The ordered pairs of mutator kinds a slice runs.  The two ACC slices run every pair that does not involve the yaw
    parameters (they change nothing without a yaw flag); the yaw slice runs every pair that involves a yaw or potential
    kind (the scope of the pair kernel).  Together: every ordered pair of the alphabet."""
    if slice_name == "2d_yaw_pot":
        return [(a, b) for a in MUTATORS for b in MUTATORS if a in YAW_SLICE_KINDS or b in YAW_SLICE_KINDS]
    return [(a, b) for a in MUTATORS for b in MUTATORS if a not in YAW_ONLY and b not in YAW_ONLY]


@functools.lru_cache(maxsize=None)
def pair_plan(slice_name, a, b):
    w = world(slice_name)
    # warm state: map + region + goal; a potential map where the slice or one of the two kinds needs one to have an effect
    pot = slice_name == "2d_yaw_pot" or a in NEED_POTENTIAL or b in NEED_POTENTIAL
    m = w.warm(potential=pot)
    warm = m.copy()
    rot = MUTATORS.index(a) * len(MUTATORS) + MUTATORS.index(b)
    steps = []
    for j, kind in enumerate((a, b)):
        op, eff = make_step(w, m, kind, rot + j)
        steps.append((op, m.copy(), eff))
    return Plan(slice_name, warm, steps, "%s>%s" % (a, b))


@functools.lru_cache(maxsize=None)
def service_plan(slice_name, kind):
    """Service table: warm state without a potential map (the resident kernel serves no other), one mutator."""
    w = world(slice_name)
    m = w.warm(potential=False)
    warm = m.copy()
    op, eff = make_step(w, m, kind, MUTATORS.index(kind))
    return Plan(slice_name, warm, [(op, m.copy(), eff)], kind)


def neutral_op(kind, rng):
    if kind == "route":
        r = ["auto", "dense", "tile", "grid"][int(rng.integers(0, 4))]
        return Op(kind, ("route", r), r)
    if kind == "service":
        mode = int(rng.integers(0, 2))
        return Op(kind, ("service", mode), str(mode))
    return Op(kind, (kind,), "")


RANDOM_PLANS = [  # (slice, seed, steps, theme)
    ("2d_acc", 1, 14, "mixed"), ("2d_acc", 2, 14, "geometry"), ("2d_acc", 3, 14, "tables"),
    ("3d_acc", 4, 12, "mixed"), ("3d_acc", 5, 12, "geometry"), ("2d_yaw_pot", 6, 12, "mixed"),
]


@functools.lru_cache(maxsize=None)
def random_plan(slice_name, seed, n_steps, theme):
    """Seeded sequence of mutators and neutral operations.  Themes: "geometry" crosses map sizes (a larger map after a
    smaller one and back: the context's buffers are re-ensured), "tables" alternates control tables of different nU on
    the same list buffers, "mixed" draws from the whole alphabet."""
    w = world(slice_name)
    rng = np.random.default_rng(7000 + seed)
    m = w.warm(potential=slice_name == "2d_yaw_pot")
    warm = m.copy()
    kinds = [k for k in MUTATORS if w.yaw or k not in YAW_ONLY]
    ptr = 5 * seed  # the plans walk the alphabet from different starts: together they reach every kind
    steps = []
    for j in range(n_steps):
        if j % 3 == 2:
            op = neutral_op(NEUTRALS[(seed + j // 3) % len(NEUTRALS)], rng)
            steps.append((op, m.copy(), None))
            continue
        if theme == "geometry" and j % 3 == 0:
            kind = ("setmap_size", "setmap_res", "setmap_origin")[(j // 3) % 3]
        elif theme == "tables" and j % 3 == 0:
            name, U = w.tables[1 - (j // 3) % 2]  # the second table, the base table, the second table, ...
            op = Op("u_table", ("set_u", U), name)
            after = apply_to_model(m.copy(), op)
            steps.append((op, after, effect(m, after, op, w.small)))
            m = after.copy()
            continue
        else:
            kind = kinds[ptr % len(kinds)]
            ptr += 1
        op, eff = make_step(w, m, kind, int(rng.integers(0, 64)))
        steps.append((op, m.copy(), eff))
    return Plan(slice_name, warm, steps, "seed%d_%s" % (seed, theme))
