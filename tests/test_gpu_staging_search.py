"""The staging walk of tests/test_gpu_staging.py, over the objects of the device search: node tables, open sets, goal
distance fields, reservation tables and the conflicts of action chains.  Every host-pointer call of mplx_table.h,
mplx_multi.h, mplx_field.h, mplx_reserve.h and mplx_traj_conflicts carves the ONE staging block of its context
(csrc/mplx_ctx.h, StageLayout); here they share it on a long-lived context whose objects live as long as it does.

One long-lived context per configuration runs a fixed order of steps on objects it keeps: one node table and open set
per number of queries a step needs (created at the first such step, node capacity 1000), one field, one reservation
table, one poly.  After every step its output equals, byte for byte, what a context created for that step alone returns
for the same inputs on objects created for that step at the smallest legal capacity.  Every host output row is filled
with the same poison in both contexts before the call (path rows past the count, the whole field download, every row
of mplx_reserve_positions, conflict rows and the columns past K of the pair matrix).  No tolerance anywhere.  Two rows
are cut to what the headers define before the comparison: the rows of a frontier past its count (mplx_table.h: "the next
frontier = the nodes improved in this call"; only the first count rows are read) and `f` of a node that was never pushed
(mplx_open.h: "Both are zero / unspecified for a node that was never pushed": f is cleared where flags lacks
MPLX_OPEN_SEEN).

State that persists by design is reset with the header's own call at the start of a step on the long-lived context:
mplx_table_clear and mplx_open_clear ("Empties the table and its status", "call it whenever the table is cleared"); a
field in force is dropped by the mplx_open_set_goals every open-set step makes (mplx_field.h: "in force until
mplx_open_clear_field, or until mplx_open_set_goals"); a reservation table, its queries and a poly are overwritten by the
step's own fill / set_queries / solve.

Steps whose call reads what an earlier host call left in an object -- table_find and table_path (the table a seed
filled), open_set_field (the field mplx_field_build made), reserve_fill_poly (the poly mplx_solve filled),
reserve_set_queries (the table mplx_reserve_fill_traj filled) -- run, on odd visits and on the long-lived context only,
two mplx_read_cells calls (n = 1000, n = 1) between the two: tests/staging_walk.py, disturb().

Where a call has a _device twin (find, the fills, the conflicts) the twin runs on the long-lived context on uploaded
copies of the inputs into poisoned device rows and returns the same bytes: these calls define every byte of their rows.

Sizes, order and poison: as tests/test_gpu_staging.py says.  Two kinds of that walk, expand_lists and read_cells, are in
this kind list unchanged."""
import ctypes as C

import numpy as np
import pytest

import field_model as FM
import staging_walk as SW
import test_gpu_field as FT
import test_gpu_staging as OLD
import test_gpu_staging_sets as SETS
from motion_primitive_library_amd import workloads as W
from staging_walk import POISON, SIZES, assert_same_bytes, fill, poisoned, ptr

SEED = 20261021
H = 3                      # horizon of the action chains
N_INSTANTS, STEP = 9, 0.3  # of a reservation table
CONFLICT_INSTANTS, CONFLICT_STEP = 40, 0.12
PATH_CAP = 70
CHECK_ROWS, CHECK_S, CHECK_B = 37, 9, 15
OLD_KINDS = ("expand_lists", "read_cells")
NEW_KINDS = ("table_seed", "table_find", "table_path", "open_set_goals", "field_build", "open_set_field", "reserve_fill_traj",
             "reserve_fill_poly", "reserve_set_queries", "traj_conflicts")
KINDS = NEW_KINDS[:5] + OLD_KINDS[:1] + NEW_KINDS[5:] + OLD_KINDS[1:]
ENTRY_POINTS = {"table_seed": ("mplx_table_seed", "mplx_table_seed_multi"), "table_find": ("mplx_table_find", "mplx_table_find_multi"),
                "table_path": ("mplx_table_path",), "open_set_goals": ("mplx_open_set_goals",), "field_build": ("mplx_field_build",),
                "open_set_field": ("mplx_open_set_field",), "reserve_fill_traj": ("mplx_reserve_fill_traj",),
                "reserve_fill_poly": ("mplx_reserve_fill_poly",), "reserve_set_queries": (), "traj_conflicts": ("mplx_traj_conflicts",)}
EMPTY, BAD_ACTION, BAD_TIME, BAD_INPUT = 1, 2, 2, 128
SEEN, IS_GOAL = 4, 2
MULTI_Q = 3  # queries of the multi form of seed and find


def schedule():
    return SW.schedule(KINDS, SEED)


def variant(kind, visit):
    if kind in ("table_seed", "table_find"):
        return visit % 2 == 1, (visit // 4) % 2 == 0, (visit // 2) % 2 == 1   # multi, g given, a stride above n
    if kind in ("reserve_fill_traj", "reserve_fill_poly"):
        return tuple(1 - ((visit >> b) & 1) for b in range(3)) + ((visit // 2) % 2,)   # t0, radius, group present; mode
    if kind == "reserve_set_queries":
        return (visit % 2 == 0,)                                          # ignore groups given
    if kind == "traj_conflicts":
        return SETS.variant("poly_conflicts", visit)
    return ()


def queries_of(kind, n, visit):
    """The number of queries of the table a step runs on."""
    if kind in ("table_seed", "table_find"):
        return MULTI_Q if variant(kind, visit)[0] else 1
    if kind in ("open_set_goals", "open_set_field"):
        return min(n, 65536)   # mplx_multi.h: n_queries in [1, 65536]
    if kind == "reserve_set_queries":
        return min(n, 64)
    return 1


# ---- CPU: the order, the variants, what the inputs hold
def test_the_order_runs_every_kind_at_every_size():
    steps = schedule()
    assert {(kind, n) for kind, n, _ in steps} == {(kind, n) for kind in KINDS for n in SIZES}
    sizes = [n for _, n, _ in steps]
    assert any(a == 3 and b == 1000 for a, b in zip(sizes, sizes[1:])) and any(a == 1000 and b == 3 for a, b in zip(sizes, sizes[1:]))
    for kind in KINDS:
        assert [visit for k, _, visit in steps if k == kind] == list(range(sum(k == kind for k, _, _ in steps))), kind
    assert steps == schedule(), "the order must not depend on the run"
    reached = {kind: {variant(kind, visit) for k, _, visit in steps if k == kind} for kind in NEW_KINDS}
    for kind in ("table_seed", "table_find"):
        assert reached[kind] == {(m, g, s) for m in (False, True) for g in (False, True) for s in (False, True)}, kind
    for kind in ("reserve_fill_traj", "reserve_fill_poly"):
        assert {v[:3] for v in reached[kind]} == {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}, kind
        assert {v[3] for v in reached[kind]} == {0, 1}
    assert reached["reserve_set_queries"] == {(False,), (True,)}
    assert {v[0] for v in reached["traj_conflicts"]} == set(SETS.CONFLICT_VARIANTS)
    for kind in ("table_find", "table_path", "open_set_field", "reserve_fill_poly", "reserve_set_queries"):
        assert {visit % 2 for k, n, visit in steps if k == kind and n == SIZES[-1]} == {0, 1}, kind   # with and without disturb()
    assert {queries_of(k, n, v) for k, n, v in steps} == {1, 3, 64, 65, 257, 1000}


def test_every_kind_runs_directly_after_every_other_kinds_largest_size():
    steps = schedule()
    after = {(a, b) for (a, n, _), (b, _, _) in zip(steps, steps[1:]) if n == SIZES[-1] and a != b}
    assert after == {(a, b) for a in KINDS for b in KINDS if a != b}
    for kind in NEW_KINDS:
        assert any((old, kind) in after for old in OLD_KINDS) and any((kind, old) in after for old in OLD_KINDS)


@pytest.mark.parametrize("config", sorted(SW.CONFIGS))
def test_every_step_has_kept_and_excluded_items(config):
    """What tests/field_model.py, tests/conflict_model.py and the headers say of the inputs, without a device."""
    import conflict_model as CM
    w = World(config)
    # field 0 of every build is the corner box of boxes(): cells it reaches and cells it does not
    lo, hi = FT.boxes(0, list(w.map_dim), 3)
    d0 = FM.field(FM.blocked_of(w.cells.ravel()), list(w.map_dim), lo[0], hi[0])
    assert (d0 == -1).any() and (d0 > 0).any()
    for i, (kind, n, visit) in enumerate(schedule()):
        if kind in OLD_KINDS or n < 65:
            continue
        x = w.inputs(i, kind, n, visit)
        if kind in ("reserve_fill_traj", "traj_conflicts"):
            st = x["predicted"]
            assert (st == 0).mean() >= 0.1 and (st & EMPTY).any() and (st & BAD_ACTION).any(), (i, kind)
            ok = CM.inputs_ok(n, x["t0"] if x["use"][0] else None, x["radius"] if x["use"][1] else x["radius_all"])
            assert bool((~ok).any()) == bool(x["use"][1] or x["use"][0]), (i, kind)
        if kind == "reserve_fill_poly":
            st = x["sets"]["predicted"]["solve"]
            assert (st == 0).mean() >= 0.1 and (st & EMPTY).any() and (st & BAD_TIME).any(), (i, kind)
        if kind == "table_find":
            assert x["n_seed"] >= 1 and n - (n + 1) // 2 >= 1


# ---- the inputs of a step (numpy only; the same for both contexts and the twin)
class World(SETS.World):
    def chains(self, rng, i, n):
        """n action chains of up to H primitives from free cells: empty chains, bad actions, two robots on one path (a
        conflict by construction) and one far from everybody (none)."""
        k = np.arange(n)
        starts = W.random_frontier(self.cells, self.origin, self.res, n, SEED + i, self.control, 2.0, 0.5)
        starts[self.F - 1] = 0.0
        actions = rng.integers(0, self.nU, size=(H, n)).astype(np.int32)
        cut = rng.integers(1, H + 1, size=n)
        actions[np.arange(H)[:, None] >= cut[None, :]] = -1
        actions[0, k % 13 == 3] = -1                 # MPLX_TRAJ_EMPTY
        actions[1, k % 13 == 7] = self.nU + 5        # MPLX_TRAJ_BAD_ACTION
        actions[0, k % 13 == 7] = 0
        if n > 2:
            starts[:, 2], actions[:, 2] = starts[:, 1], actions[:, 1]
        if n > 4:
            starts[0, 4] += 100.0
        first = actions[0]
        bad = ((actions < -1) | (actions >= self.nU))
        status = np.where(first == -1, EMPTY, 0) | np.where(bad.any(axis=0) & (first != -1), BAD_ACTION, 0)
        status = np.where(bad[0], EMPTY | BAD_ACTION, status)
        return np.ascontiguousarray(starts), np.ascontiguousarray(actions), status.astype(np.uint8)

    def clock(self, rng, n):
        k = np.arange(n)
        r0 = 0.15 * (float(np.prod(self.extent())) / max(n, 65)) ** (1.0 / self.dim)
        t0 = rng.uniform(-0.5, 1.0, size=n)
        t0[:min(n, 3)] = 0.0
        t0[k % 17 == 5] = np.array([np.nan, np.inf])[(k[k % 17 == 5] // 17) % 2]
        radius = rng.uniform(0.5, 1.5, size=n) * r0
        radius[k % 17 == 11] = -1.0
        return dict(t0=t0, radius=radius, radius_all=r0, group=(k % 5).astype(np.int32), rank=rng.integers(0, 4, size=n).astype(np.int32))

    def inputs(self, i, kind, n, visit):
        if kind in OLD_KINDS:
            return OLD.World.inputs(self, i, kind, n, visit)
        rng = np.random.default_rng(SEED + i)
        x = {"Q": queries_of(kind, n, visit)}
        k = np.arange(n)
        if kind in ("table_seed", "table_find", "open_set_goals", "open_set_field"):
            multi, with_g, wide = variant(kind, visit) if kind.startswith("table") else (True, False, False)
            m = max(1, n // 2) if kind == "table_find" else n
            stride = m + 3 if wide else m
            st = W.random_frontier(self.cells, self.origin, self.res, m, SEED + i, self.control, 2.0, 0.5)
            src = np.where(k % 3 == 2, k // 3, k) if kind == "table_seed" else np.arange(m)   # duplicates among the seeds (of one query)
            st = st[:, src]
            states = np.zeros((self.F, stride))
            states[:, :m] = st
            x.update(states=states, n_seed=m, stride=stride, g=rng.choice([0.0, 0.5, 1.0, 2.5], size=m) if with_g else None,
                     query=(src % x["Q"]).astype(np.int32) if (multi or x["Q"] > 1) else None)
        if kind in ("open_set_goals", "open_set_field"):
            goals = W.random_frontier(self.cells, self.origin, self.res, n, SEED + 7919 + i, self.control, 2.0, 0.5).T.copy()
            goals[k % 4 == 0] = x["states"][:, :n].T[k % 4 == 0]             # every fourth query starts inside its goal region
            x.update(goals=np.ascontiguousarray(goals), tol=0.3 + 0.1 * (k % 3))
        if kind in ("field_build", "open_set_field"):
            F = n if kind == "field_build" else min(n, 8)
            lo, hi = FT.boxes(SEED + i, list(self.map_dim), F)
            x.update(F=F, lo=np.ascontiguousarray(lo, dtype=np.int32), hi=np.ascontiguousarray(hi, dtype=np.int32),
                     field_of_query=((k % (F + 1)) - 1).astype(np.int32))
        if kind == "table_path":
            L = min(n, 64)
            j = np.arange(L)
            x.update(L=L, seed=W.random_frontier(self.cells, self.origin, self.res, 1, SEED + i, self.control, 2.0, 0.5),
                     count=np.ones(L, np.int32), action=((j * 7) % self.nU).astype(np.int32), cost=np.full(L, 0.5),
                     hash=((j.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1),
                     state=rng.standard_normal((self.F, L)), parent_id=j.astype(np.int32), parent_g=0.5 * j)
        if kind in ("reserve_fill_traj", "traj_conflicts"):
            starts, actions, status = self.chains(rng, i, n)
            x.update(starts=starts, actions=actions, predicted=status, **self.clock(rng, n))
            x["use"] = variant(kind, visit)[:3] if kind == "reserve_fill_traj" else variant(kind, visit)[0][:3]
        if kind == "reserve_fill_poly":
            x["sets"] = SETS.World.inputs(self, i, "poly_conflicts", n, visit)
            x.update({key: x["sets"][key] for key in ("t0", "radius", "radius_all", "group")})
            x["use"] = variant(kind, visit)[:3]
        if kind == "reserve_set_queries":
            Q = x["Q"]
            q = np.arange(Q)
            c = self.check_list()
            x["looked"] = c["live"] & np.repeat(c["parent_id"] >= 0, CHECK_S) & np.isfinite(np.where(c["live"], c["cost"], 0.0))
            x.update(q_t0=0.25 * (q % 4), q_radius=(0.2 + 0.05 * (q % 5)) * self.check_list()["rr"],
                     q_ignore=((q % 3) - 1).astype(np.int32) if variant(kind, visit)[0] else None)
        return x

    def check_list(self):
        """The fixed reservations (CHECK_B chains) and the fixed list of CHECK_ROWS rows the check of every
        reserve_set_queries step runs on: the shape of test_check_equals_the_model in tests/test_gpu_reserve.py."""
        if not hasattr(self, "_check"):
            rng = np.random.default_rng(SEED - 1)
            B, n, S, D, ext = CHECK_B, CHECK_ROWS, CHECK_S, self.dim, self.extent()
            starts, actions, _ = self.chains(rng, -1, B)
            # radii sized so that about half of the entries are blocked: B balls of radius rr fill 0.7 of the map
            rr = (0.7 * float(np.prod(ext)) / B / (np.pi if D == 2 else 4.19)) ** (1.0 / D)
            radius = rr * rng.uniform(0.4, 0.8, size=B)
            pst = np.zeros((self.F, n))
            pst[:D] = rng.uniform(0.1, 0.9, size=(D, n)) * ext[:, None]
            pst[D:2 * D] = rng.uniform(-0.3, 0.3, size=(D, n))
            pst[self.F - 1] = (np.arange(n) % 4) * 1.0   # parent times; tp = 3 leaves the horizon of 9 instants of 0.3
            count = rng.integers(0, S + 1, size=n).astype(np.int32)
            count[:3] = [S, 0, 1]
            live = (np.arange(S)[None, :] < count[:, None]).ravel()
            action = poisoned("<i4", (n * S,))
            cost = poisoned("<f8", (n * S,))
            action[live] = rng.integers(0, self.nU, size=int(live.sum()))
            cost[live] = rng.choice([0.5, 1.0, 2.0, np.inf], p=[0.3, 0.3, 0.3, 0.1], size=int(live.sum()))
            parent_id = np.arange(n, dtype=np.int32)
            parent_id[[4, 20]] = -1
            seeds = np.zeros((self.F, n))
            seeds[:D] = 0.5 + np.arange(n)[None, :] * 0.01 + np.arange(D)[:, None]   # distinct lattice states
            self._check = dict(starts=starts, actions=actions, radius=radius, t0=rng.choice([0.0, 0.5, -0.7], size=B), rr=rr, pst=pst,
                               count=count, action=action, cost=cost, parent_id=parent_id, seeds=seeds, live=live,
                               group=(np.arange(B) // 2).astype(np.int32))
        return self._check


# ---- the objects of a context
class Objects:
    def __init__(self, engine, env, capacity):
        self.engine, self.abi, self.env, self.capacity = engine, engine._abi, env, capacity
        self.tables, self._field, self._reserve, self._polys = {}, None, None, None

    def table(self, Q):
        """(table, open set) of Q queries: created at the first step that needs them, kept from then on."""
        if Q not in self.tables:
            tab = self.engine.NodeTable(self.env, self.capacity, n_queries=Q)
            self.tables[Q] = (tab, self.engine.OpenSet(self.env, tab))
        return self.tables[Q]

    def field(self):
        if self._field is None:
            self._field = self.engine.search.GoalField(self.env)
        return self._field

    def reserve(self):
        if self._reserve is None:
            self._reserve = SW.handle(self.abi, self.env._ctx, self.abi.lib().mplx_reserve_create, self.env._ctx)
        return self._reserve

    def polys(self):
        if self._polys is None:
            self._polys = SETS.Polys(self.abi, self.env, self.capacity, "poly_info")
        return self._polys

    def free(self):
        for tab, opn in self.tables.values():
            opn.free()
            tab.free()
        if self._field is not None:
            self._field.free()
        if self._reserve is not None:
            self.abi.lib().mplx_reserve_destroy(self._reserve)
        if self._polys is not None:
            self._polys.free()
        self.tables, self._field, self._reserve, self._polys = {}, None, None, None


def frontier(o, capacity):
    """A frontier whose every row holds the poison."""
    fr = o.engine.TableFrontier(o.env, capacity)
    for b in (fr.id, fr.g, fr.state, fr.count):
        o.abi.check(o.env._ctx, o.abi.lib().mplx_memset(o.env._ctx, b.ptr, POISON, b.nbytes))
    return fr


def seed(o, tab, x, fr, count):
    L = o.abi.lib()
    f = fr.c_struct()
    n, cnt = x["n_seed"], C.cast(count.ctypes.data, C.POINTER(C.c_int64))
    if x["query"] is None:
        rc = L.mplx_table_seed(tab._tab, ptr(x["states"]), n, x["stride"], ptr(x["g"]), C.byref(f), cnt)
    else:
        rc = L.mplx_table_seed_multi(tab._tab, ptr(x["states"]), n, x["stride"], ptr(x["g"]), ptr(x["query"]), C.byref(f), cnt)
    o.abi.check(o.env._ctx, rc)


def conflict_in(abi, x, I, mode, instants, step, rank=False, chunk=0):
    ut, ur, ug = x["use"]
    return fill(abi.ConflictIn(), {}, step=step, n_steps=instants, mode=mode, t0=I["t0"] if ut else None, radius=I["radius"] if ur else None,
                radius_all=x["radius_all"], group=I["group"] if ug else None, rank=I["rank"] if rank else None, chunk_steps=chunk)


def chain_set(abi, n, I):
    return fill(abi.TrajSet(), {}, starts=I["starts"], n_starts=n, start_stride=n, actions=I["actions"], n_traj=n, horizon=H, action_stride=n)


def positions(o, w, B, instants):
    """mplx_reserve_positions into poisoned rows."""
    out = {"pos": poisoned("<f8", (instants, w.dim, B)), "active": poisoned("u1", (instants, B)), "included": poisoned("u1", (B,)),
           "radius": poisoned("<f8", (B,)), "group": poisoned("<i4", (B,)), "status": poisoned("u1", (B,))}
    o.abi.check(o.env._ctx, o.abi.lib().mplx_reserve_positions(o.reserve(), *[out[k].ctypes.data for k in
                                                                              ("pos", "active", "included", "radius", "group", "status")]))
    return out


def open_rows(opn):
    d = opn.download()
    return {"open_f": np.where(d["flags"] & SEEN, d["f"], 0.0), "open_flags": d["flags"]}


def conflict_spec(n, wide):
    s = {"first_step": ("<i4", (n,)), "first_partner": ("<i4", (n,)), "min_d2": ("<f8", (n,)), "status": ("u1", (n,))}
    if n <= 257:
        s["pair_first"] = ("<i4", (n, n + 5 if wide else n))
    return s


def host_step(o, w, kind, n, visit, x, long_lived):
    """The step on one context: name -> row."""
    abi, env, L = o.abi, o.env, o.abi.lib()
    ctx, out = env._ctx, {}
    between = long_lived and visit % 2 == 1
    I = {k: ptr(v) for k, v in x.items() if isinstance(v, np.ndarray)}
    tab = opn = None
    if kind.startswith(("table", "open")) or kind == "reserve_set_queries":
        tab, opn = o.table(x["Q"])
        tab.clear()
        opn.clear()
    if kind in ("table_seed", "table_find", "open_set_goals", "open_set_field"):
        fr, count = frontier(o, x["n_seed"]), poisoned("<i8", (1,))
        if kind == "open_set_field":
            o.field().build_boxes(x["lo"], x["hi"])
            if between:
                SW.disturb(abi, env, w.cells.size)
        seed(o, tab, x, fr, count)
        if kind == "table_seed":
            rows, t = fr.download(int(count[0])), tab.download()
            out.update(count=count, fr_id=rows["id"], fr_g=rows["g"], fr_state=rows["state"], n_nodes=np.int64(t["n_nodes"]),
                       status=np.uint32(t["status"]), **{"tab_" + k: t[k] for k in ("hash", "g", "pred", "pred_action", "query", "state")})
        elif kind == "table_find":
            if between:
                SW.disturb(abi, env, w.cells.size)
            t = tab.download()
            i = np.arange(n)
            present = i % 2 == 0
            x["find_hash"] = np.where(present, t["hash"][(i // 2) % t["n_nodes"]], ((i.astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1))
            x["find_query"] = np.where(present, t["query"][(i // 2) % t["n_nodes"]], i % x["Q"]).astype(np.int32)
            ids = poisoned("<i4", (n,))
            if x["query"] is None:
                rc = L.mplx_table_find(tab._tab, ptr(x["find_hash"]), n, ptr(ids))
            else:
                rc = L.mplx_table_find_multi(tab._tab, ptr(x["find_hash"]), ptr(x["find_query"]), n, ptr(ids))
            abi.check(ctx, rc)
            out.update(ids=ids, tab_hash=t["hash"], find_hash=x["find_hash"])
        else:
            opn.set_goals(x["goals"], tol_pos=x["tol"])
            if kind == "open_set_field":
                opn.set_field(o.field(), x["field_of_query"])
            opn.push(fr, x["n_seed"], eps=1.0)
            out.update(open_rows(opn))
            out["count"] = count
        fr.free()
    elif kind == "table_path":
        n_rows = x["L"]
        fr, count = frontier(o, n_rows), poisoned("<i8", (1,))
        seed(o, tab, dict(states=x["seed"], n_seed=1, stride=1, g=None, query=None), fr, count)
        lists = o.engine.Lists(env, n_rows, w.nU, want_state=True, stride=1, state_pad=0)
        for name in ("count", "action", "cost", "hash", "state"):
            getattr(lists, name).upload(np.ascontiguousarray(x[name]))
        dev = SW.Device(o.engine, env)
        cnt = C.c_int64(-1)
        s, f = lists.c_struct(), fr.c_struct()
        abi.check(ctx, L.mplx_table_relax_device(tab._tab, C.byref(s), n_rows, dev.up(x["parent_id"]), dev.up(x["parent_g"]), float("inf"),
                                                  C.byref(f), None, C.byref(cnt)))
        if between:
            SW.disturb(abi, env, w.cells.size)
        ids, act, edges = poisoned("<i4", (PATH_CAP + 1,)), poisoned("<i4", (PATH_CAP,)), poisoned("<i8", (1,))
        abi.check(ctx, L.mplx_table_path(tab._tab, n_rows, ptr(ids), ptr(act), PATH_CAP, C.cast(edges.ctypes.data, C.POINTER(C.c_int64))))
        out.update(ids=ids, actions=act, n_edges=edges, relaxed=np.int64(cnt.value))
        dev.free()
        lists.free()
        fr.free()
    elif kind == "field_build":
        fld = o.field()
        fld.build_boxes(x["lo"], x["hi"])
        dist = poisoned("<i4", (x["F"], w.cells.size))
        abi.check(ctx, L.mplx_field_download(fld._fld, ptr(dist)))
        out.update(dist=dist, shape=np.array(fld.shape, np.int64))
    elif kind == "reserve_fill_traj":
        s, i = chain_set(abi, n, I), conflict_in(abi, x, I, variant(kind, visit)[3], N_INSTANTS, STEP)
        abi.check(ctx, L.mplx_reserve_fill_traj(o.reserve(), ctx, C.byref(s), C.byref(i)))
        out.update(positions(o, w, n, N_INSTANTS))
    elif kind == "reserve_fill_poly":
        xs, polys = x["sets"], o.polys()
        got, P = SETS.host_rows(SETS.out_spec(w, "solve_device", n, visit, xs))
        SETS.call(abi, polys, w, "solve", n, visit, xs, P, {k: ptr(xs[k]) for k in ("wp", "n_wp", "dts", "v_arr", "flags")})
        out.update({"set_" + k: v for k, v in got.items()})
        if between:
            SW.disturb(abi, env, w.cells.size)
        i = conflict_in(abi, x, I, variant(kind, visit)[3], N_INSTANTS, STEP)
        abi.check(ctx, L.mplx_reserve_fill_poly(o.reserve(), polys.h["a"], C.byref(i)))
        out.update(positions(o, w, n, N_INSTANTS))
    elif kind == "reserve_set_queries":
        c, Q = w.check_list(), x["Q"]
        Ic = {k: ptr(v) for k, v in c.items() if isinstance(v, np.ndarray)}
        s = chain_set(abi, CHECK_B, Ic)
        i = fill(abi.ConflictIn(), {}, step=STEP, n_steps=N_INSTANTS, mode=visit % 2, t0=Ic["t0"], radius=Ic["radius"], group=Ic["group"])
        abi.check(ctx, L.mplx_reserve_fill_traj(o.reserve(), ctx, C.byref(s), C.byref(i)))
        if between:
            SW.disturb(abi, env, w.cells.size)
        abi.check(ctx, L.mplx_reserve_set_queries(o.reserve(), Q, ptr(x["q_t0"]), ptr(x["q_radius"]), ptr(x["q_ignore"])))
        fr, count = frontier(o, CHECK_ROWS), poisoned("<i8", (1,))
        if Q > 1:  # whose the rows are: node k = seed k, of query k mod Q
            seed(o, tab, dict(states=c["seeds"], n_seed=CHECK_ROWS, stride=CHECK_ROWS, g=None, query=(np.arange(CHECK_ROWS) % Q).astype(np.int32)),
                 fr, count)
            assert int(count[0]) == CHECK_ROWS
        lists = o.engine.Lists(env, CHECK_ROWS, w.nU, want_state=False, stride=CHECK_S)
        for name in ("count", "action", "cost"):
            getattr(lists, name).upload(c[name])
        dev = SW.Device(o.engine, env)
        hit = dev.rows({"hit": ("<i8", (CHECK_ROWS * CHECK_S,))})["hit"]
        sl = lists.c_struct()
        abi.check(ctx, L.mplx_reserve_check_device(o.reserve(), tab._tab if Q > 1 else None, C.byref(sl), CHECK_ROWS, dev.up(c["parent_id"]),
                                                    dev.up(c["pst"]), CHECK_ROWS, hit, None))
        out.update(dev.download())
        out["cost"] = lists.cost.download(np.float64, (CHECK_ROWS * CHECK_S,))
        dev.free()
        lists.free()
        fr.free()
    else:
        assert kind == "traj_conflicts", kind
        _, mode, chunk, wide = variant(kind, visit)
        got, P = SETS.host_rows(conflict_spec(n, wide))
        i = conflict_in(abi, x, I, mode, CONFLICT_INSTANTS, CONFLICT_STEP, rank=variant(kind, visit)[0][3], chunk=chunk)
        s = chain_set(abi, n, I)
        abi.check(ctx, L.mplx_traj_conflicts(ctx, C.byref(s), C.byref(i), C.byref(fill(abi.ConflictOut(), P, pair_stride=n + 5 if wide else n))))
        out.update(got)
    return out


def twin_step(o, w, kind, n, visit, x):
    """The _device form of the call of a step on the long-lived context, where there is one: name -> row, or None."""
    abi, env, L = o.abi, o.env, o.abi.lib()
    ctx = env._ctx
    dev = SW.Device(o.engine, env)
    try:
        if kind == "table_find":
            tab, _ = o.table(x["Q"])
            ids = dev.rows({"ids": ("<i4", (n,))})["ids"]
            if x["query"] is None:
                rc = L.mplx_table_find_device(tab._tab, dev.up(x["find_hash"]), n, ids)
            else:
                rc = L.mplx_table_find_multi_device(tab._tab, dev.up(x["find_hash"]), dev.up(x["find_query"]), n, ids)
            abi.check(ctx, rc)
            return dev.download()
        if kind in ("reserve_fill_traj", "reserve_fill_poly"):
            I = {k: dev.up(x[k]) for k in ("t0", "radius", "group") + (("starts", "actions") if kind == "reserve_fill_traj" else ())}
            i = conflict_in(abi, x, I, variant(kind, visit)[3], N_INSTANTS, STEP)
            if kind == "reserve_fill_traj":
                s = chain_set(abi, n, I)
                abi.check(ctx, L.mplx_reserve_fill_traj_device(o.reserve(), ctx, C.byref(s), C.byref(i)))
            else:
                abi.check(ctx, L.mplx_reserve_fill_poly_device(o.reserve(), o.polys().h["a"], C.byref(i)))
            env.synchronize()
            return positions(o, w, n, N_INSTANTS)
        if kind == "traj_conflicts":
            _, mode, chunk, wide = variant(kind, visit)
            I = {k: dev.up(x[k]) for k in ("t0", "radius", "group", "rank", "starts", "actions")}
            P = dev.rows(conflict_spec(n, wide))
            i = conflict_in(abi, x, I, mode, CONFLICT_INSTANTS, CONFLICT_STEP, rank=variant(kind, visit)[0][3], chunk=chunk)
            s = chain_set(abi, n, I)
            abi.check(ctx, L.mplx_traj_conflicts_device(ctx, C.byref(s), C.byref(i), C.byref(fill(abi.ConflictOut(), P, pair_stride=n + 5 if wide else n))))
            return dev.download()
        return None
    finally:
        dev.free()


def assert_not_vacuous(kind, n, x, want, what):
    """On the output of the fresh context, the reference."""
    if kind == "field_build":
        assert (want["dist"] == -1).any() and (want["dist"] >= 0).any(), what + ": a field without -1 or without finite cells"
    if kind == "table_find" and n >= 3:
        assert (want["ids"] >= 0).any() and (want["ids"] == -1).any(), what + ": nothing found, or everything"
        assert np.array_equal(want["ids"] >= 0, np.arange(n) % 2 == 0), what
    if kind == "table_path":
        assert int(want["n_edges"][0]) == x["L"] and np.array_equal(want["ids"][:x["L"] + 1], np.arange(x["L"] + 1)), what
    if kind == "table_seed":
        assert 0 < int(want["n_nodes"]) == int(want["count"][0]) <= n and (n < 3 or int(want["n_nodes"]) < n), what + ": no duplicate among the seeds"
    if kind == "reserve_set_queries":
        looked = want["hit"][x["looked"]]   # (-1 is also what an entry that is not looked at gets)
        assert (looked >= 0).any() and (looked == -1).any(), what + ": the check has no hit, or no miss"
    if n < 65:
        return
    if kind in ("open_set_goals", "open_set_field"):
        assert (want["open_flags"] & IS_GOAL).any() and not (want["open_flags"] & IS_GOAL).all(), what
    if kind == "open_set_field":
        assert np.isinf(want["open_f"]).any() and np.isfinite(want["open_f"]).any(), what
    if kind in ("reserve_fill_traj", "traj_conflicts"):
        st = want["status"]
        assert np.array_equal(st & (EMPTY | BAD_ACTION), x["predicted"]), what + ": not the statuses mplx_traj.h gives these chains"
        assert (st == 0).mean() >= 0.1 and (st & EMPTY).any() and (st & BAD_ACTION).any(), what
        assert bool((st & BAD_INPUT).any()) == bool(x["use"][0] or x["use"][1]), what
    if kind == "reserve_fill_poly":
        st = want["status"]
        assert np.array_equal(st & 3, x["sets"]["predicted"]["solve"]), what
        assert (st == 0).mean() >= 0.1 and (st & EMPTY).any() and (st & BAD_TIME).any(), what
        assert bool((st & BAD_INPUT).any()) == bool(x["use"][0] or x["use"][1]), what
    if kind.startswith("reserve_fill"):
        assert want["included"].any() and not want["included"].all(), what
    if kind == "traj_conflicts":
        included = (want["status"] == 0)
        assert (want["first_step"][included] >= 0).any() and (want["first_step"][included] == -1).any(), what + ": no hit, or no miss"


@pytest.mark.gpu
@pytest.mark.parametrize("config", sorted(SW.CONFIGS))
def test_search_objects_share_the_staging_block_of_a_long_lived_context(engine, monkeypatch, config):
    monkeypatch.setenv("MPLX_ARENA_KB", "1")  # read by mplx_create: every lists batch takes the large path
    abi, w = engine._abi, World(config)
    env = engine.EnvMap(w.dim, 0)
    w.configure(env)
    kept = Objects(engine, env, SIZES[-1])
    stats = {}
    for i, (kind, n, visit) in enumerate(schedule()):
        what = "%s step %d: %s n=%d visit %d" % (config, i, kind, n, visit)
        x = w.inputs(i, kind, n, visit)
        fresh = engine.EnvMap(w.dim, 0)
        w.configure(fresh)
        if kind in OLD_KINDS:
            want = OLD.host_call(abi, fresh, w, kind, n, x)
            fresh.close()
            got = OLD.host_call(abi, env, w, kind, n, x)
            assert_same_bytes(got, want, what)
            if kind in OLD.TWINNED:
                OLD.assert_equals_twin(w, kind, n, got, OLD.device_call(engine, env, w, kind, n, x), what)
            stats.setdefault(kind, []).append((n, None))
            continue
        own = Objects(engine, fresh, {"table_path": min(n, 64) + 1, "reserve_set_queries": CHECK_ROWS}.get(kind, n))
        want = host_step(own, w, kind, n, visit, x, False)
        own.free()
        fresh.close()
        assert_not_vacuous(kind, n, x, want, what)
        got = host_step(kept, w, kind, n, visit, x, True)
        assert_same_bytes(got, want, what)
        twin = twin_step(kept, w, kind, n, visit, x)
        if twin is not None:
            assert_same_bytes(twin, {k: got[k] for k in twin}, what + ", the _device form")
        row = want.get("status") if kind not in ("table_seed",) else None
        stats.setdefault(kind, []).append((n, None if row is None else float((row == 0).mean())))
    kept.free()
    env.close()
    for kind in KINDS:
        at_1000 = [s for n, s in stats[kind] if n == SIZES[-1] and s is not None]
        print("%s %-20s steps %3d  status 0 at n = 1000: %s" % (config, kind, len(stats[kind]),
              "%.3f .. %.3f" % (min(at_1000), max(at_1000)) if at_1000 else "-"))
