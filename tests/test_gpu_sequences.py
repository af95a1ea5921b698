"""A long-lived context through sequences of setters against a context built from scratch in the final state.

Every other parity test configures a fresh context once.  A planner keeps one context for hours and changes it all the
time, and the context (csrc/mplx_ctx.h) carries state that is DERIVED from what the setters were given and must be
invalidated by exactly the right calls:

| derived state | made from | invalidated / guarded by |
|---|---|---|
| blocked bits `blk`, `blk_ok` | map or potential map, region bits | set_map, set_potential, set_region, update_potential_map, set_search_region_path, map_dilate, map_free, comm_broadcast_map; patched in place by edit_map (only without a potential map) |
| summed-area table `sat`, `sat_ok`, `sat_stale` | `blk` | rebuilt with `blk`; switched off by edit_map, rebuilt by the first launch of >= 4096 nodes (lists_device) |
| sample tables `tables_ok`, `tab_dt`, `tab_res`, `recips` | prm.dt, res | compared on use (ensure_tables) |
| control factorisation `u_factored / u_wide / u_lex / u_nd / uvals / uidx / h_uyaw / u_absmax` | control table | set_controls -- but whether the kernels may take `u_lex` also depends on the FLAG in force at the launch: a table with a yaw-rate column is nested-loop order over four factors, and under a flag without yaw the lexicographic kernels enumerated three (half the successors; found and fixed with this module, plan_grid) |
| `has_pot`, `has_region` | setters | also dropped by set_map with another geometry |
| occupancy cache `grid_occ` | (control, potential, LDS) | never cleared except on overflow |
| resident service kernel `svc` (captured TileArgs: map, REGION, params, controls, goal) | the whole context at launch time | bind_device() / svc_stop() in each mutating entry point -- mplx_set_region(NULL) and mplx_set_potential(NULL) did neither (fixed with this module) |
| fused goal `goal_fuse`, `has_goal` | set_goal | stops the service when it changes |
| counters zero between launches (`work_counter`, `live_ctr`, `done_count`) | previous launch | each kernel's epilogue |
| pending yaw fix-ups `yaw_pending` | earlier launches | resolve_pending() at the top of every mutating call |
| scratch shared between operations (`prep_a`, `prep_b`, `prep_lut`; the staging block `s_arena` of every host-pointer call) | dilate, potential passes, region boxes, clouds; read / edit cells and the other host-pointer calls | ensure() grows only |
| Python mirror `EnvMap.has_potential` | Python setters | by hand -- setMap with another geometry left it True (fixed with this module) |

A new setter, or new derived state, belongs in the alphabet of tests/sequence_model.py (MUTATORS + variants()): the
tables below then run it against every other kind in both orders.

Method.  A host-side model (sequence_model.Model) holds what the context should hold; after EVERY step a fresh
oracle.Env is built from it (the reference build where it exists) and the long-lived context is observed through
  * two small host-pointer batches in a row and one get_succ: the resident service kernel where the configuration is
    eligible -- asserted through service()["requests"], so the test cannot pass by bypassing it;
  * a resident launch of 192 nodes at S = nU and at S rounded up to 32, and one of 4096 nodes (after an editMap: the
    free-box table is off for the first, rebuilt for the second), into device buffers allocated once per context at
    the largest stride with room for 8 nodes more, poisoned before every launch: what mplx.h:171-181 does not allow a
    launch to write must still be poison afterwards (past count[k] -- up to the next multiple of 32 only when S % 32
    == 0, and `action` there is -1 --, past n_nodes, unrequested rows).  The host-pointer form promises more (entries
    past count[k] untouched): same canary on the numpy arrays, service path and pipelined copy-back;
  * heur / flags rows while the model holds a goal (helpers.check_fused_rows); a launch that asks for them right after
    "clear goal" must fail with MPLX_ERR_STATE;
  * the Python mirror: has_potential, and read_cells(potential=True) failing exactly when there is none;
  * at the end of a table entry and every fourth random step: read_cells(all) of map and potential, check_edges
    against oracle.check_edges (flags without yaw, no potential map: the scope tests/test_edges.py pins), a 4096-node
    host batch.

Slices.  (a) The pairwise table runs every ordered pair of mutator KINDS (23 kinds; the variants of a kind rotate with
the pair's index) in 2D/ACC and 3D/ACC -- without the pairs of the yaw parameters, which no flag without yaw consults
-- and every pair that involves a potential-map or yaw-parameter kind under 2D ACCxYAW on a potential map, the pair
kernel's scope.  (b) The service table: resident kernel up (MPLX_SERVICE_IDLE_US = 0.5 s, so it does not leave on its
own), one mutator, two batches against the oracle and a fresh context without the service.  (c) Seeded random
sequences of mutators and neutral operations, across geometry changes and alternating control tables.

The 4096-node launch asks for every row while the table has at most 64 controls, and for count / action / cost / hash
above that (a 1100-control table at 4104 x 1120 entries x 145 bytes would be 670 MB to download per step).

The generator's own tests run without a GPU: every step of the tables can be noticed by the oracle alone (or is listed
with its reason), the pair table covers the alphabet, the canary catches planted writes, the model's chained map
operations equal the reference's.

Cost on an MI355X: 1225 GPU tests in 108 s (the existing -m gpu suite: 149 s in the same session); the pair table is
1173 of them at about 85 ms each."""
import os

import numpy as np
import pytest

import sequence_model as SM
from helpers import assert_lists_equal, check_fused_rows, require_reference_build
from oracle import oracle as O
from test_gpu_parity import YAW_COST_RTOL
from test_map_util import np_cloud, np_dilate

POISON = 0xA5
POISON_I32 = np.frombuffer(bytes([POISON] * 4), dtype=np.int32)[0]
ITEM = {"count": ("<i4", 4), "action": ("<i4", 4), "cost": ("<f8", 8), "hash": ("<u8", 8), "state": ("<f8", 8),
        "iters": ("<i4", 4), "heur": ("<f8", 8), "flags": ("u1", 1)}
EXTRA_NODES = 8


@pytest.fixture(autouse=True)
def _patient_kernel(monkeypatch):
    """The resident kernel must not leave on its idle timer between two calls of a test: whether a stale kernel answers
    is then a matter of the code, not of timing.  Read by mplx_create, so set before any context exists."""
    monkeypatch.setenv("MPLX_SERVICE_IDLE_US", "500000")


def _round32(n):
    return (int(n) + 31) & ~31


def _poisoned(dtype, shape):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = POISON
    return a


def _sub(ref, n, nU):
    out = {k: ref[k][:n * nU] for k in ("status", "cost", "hash", "iters")}
    out["state"] = ref["state"][:, :n * nU]
    return out


def _tile(ref, reps):
    out = {k: np.tile(ref[k], reps) for k in ("status", "cost", "hash", "iters")}
    out["state"] = np.tile(ref["state"], (1, reps))
    return out


class Rows:
    """Device list buffers allocated once and reused launch after launch with whatever stride the step needs."""

    def __init__(self, engine, env, cap_nodes, cap_slots, full):
        self.env, self.abi, self.cap_nodes, self.cap_slots, self.F = env, engine._abi, int(cap_nodes), int(cap_slots), env.n_fields
        self.names = ["count", "action", "cost", "hash"] + (["state", "iters", "heur", "flags"] if full else [])
        self.nbytes = {n: (self.cap_nodes if n == "count" else self.cap_slots * (self.F if n == "state" else 1)) * ITEM[n][1]
                       for n in self.names}
        self.dev = {n: engine.DeviceArray(env, self.nbytes[n]) for n in self.names}
        self.S, self.fused = 0, False

    def arm(self, S, fused):
        """Poison every row; the next launch through c_struct() uses stride S and asks for heur / flags iff `fused`."""
        for n in self.names:
            self.abi.check(self.env._ctx, self.abi.lib().mplx_memset(self.env._ctx, self.dev[n].ptr, POISON, self.nbytes[n]))
        self.S, self.fused = int(S), bool(fused)
        return self

    def c_struct(self):  # (what EnvMap.expand_lists_resident / post_lists / pack_lists ask a Lists object for)
        s = self.abi.SuccLists()
        d = self.dev
        s.count, s.action, s.cost, s.hash = d["count"].ptr, d["action"].ptr, d["cost"].ptr, d["hash"].ptr
        s.node_stride = self.S
        if "state" in d:
            s.state, s.state_stride, s.iters = d["state"].ptr, self.cap_slots, d["iters"].ptr
            if self.fused:
                s.heur, s.flags = d["heur"].ptr, d["flags"].ptr
        return s

    def read(self, n, nU, what):
        """Download every row whole, check the canary, return the lists of the first n nodes."""
        S, cap = self.S, self.cap_slots
        raw = {k: self.dev[k].download(np.uint8, (self.nbytes[k],)) for k in self.names}
        count = raw["count"].view(np.int32)[:n].copy()
        assert (raw["count"][4 * n:] == POISON).all(), "%s: count row written past n_nodes" % what
        assert ((count >= 0) & (count <= nU)).all(), "%s: count outside [0, nU]" % what
        j = np.arange(cap) % S
        cnt = np.zeros(cap, np.int64)
        cnt[:n * S] = np.repeat(count, S)
        inside = np.arange(cap) < n * S
        used = inside & (j < cnt)
        pad = inside & ~used & (S % 32 == 0) & (j < ((cnt + 31) & ~31))
        must = ~(used | pad)
        got = {"stride": S, "count": count}
        for k in self.names[1:]:
            dt, isz = ITEM[k]
            # (compared at the width of an entry: an entry is poison iff each of its bytes is)
            u = raw[k].view("<u%d" % isz)
            neq = u != np.frombuffer(bytes([POISON] * isz), dtype=u.dtype)[0]
            if k in ("heur", "flags") and not self.fused:
                assert not neq.any(), "%s: row `%s` was not asked for and was written" % (what, k)
                continue
            dirty = neq.reshape(self.F, cap) & must[None, :] if k == "state" else neq & must
            assert not dirty.any(), "%s: row `%s` written outside what a launch may write (stride %d, %d nodes): %d entries, first slot %s" % (
                what, k, S, n, int(dirty.sum()), np.argwhere(dirty)[0].tolist())
            v = raw[k].view(dt)
            got[k] = v.reshape(self.F, cap)[:, :n * S] if k == "state" else v[:n * S]
        ap = raw["action"].view(np.int32)[pad]
        assert ((ap == -1) | (ap == POISON_I32)).all(), "%s: line padding of `action` must be -1" % what
        return got

    def free(self):
        for d in self.dev.values():
            d.free()


class Driver:
    """One long-lived context, the model it should equal, and the observers."""

    def __init__(self, engine, plan, light=False):
        self.m, self._abi, self.plan = engine, engine._abi, plan
        self.w = SM.world(plan.slice)
        self.use_ref = require_reference_build()
        self.env = env = engine.EnvMap(self.w.dim, 0)
        self.model = plan.warm.copy()
        self.route, self.service_on = "auto", True
        self.configure(env, self.model)
        models = plan.models()
        s_all = max(_round32(x.nU) for x in models)
        self.light = light
        if not light:
            big = np.ascontiguousarray(np.tile(self.w.probes, (1, SM.N_BIG // SM.N_DISTINCT)))
            self.big_nodes = big
            self.fr = env.upload_frontier(big)
            self.small_rows = Rows(engine, env, SM.N_RES + EXTRA_NODES, (SM.N_RES + EXTRA_NODES) * s_all, True)
            s_full = max(_round32(x.nU) for x in models if x.nU <= SM.FULL_ROWS_MAX_NU)
            self.big_rows = Rows(engine, env, SM.N_BIG + EXTRA_NODES, (SM.N_BIG + EXTRA_NODES) * s_full, True)
            self.lean_rows = None
            if any(x.nU > SM.FULL_ROWS_MAX_NU for x in models):
                self.lean_rows = Rows(engine, env, SM.N_BIG + EXTRA_NODES, (SM.N_BIG + EXTRA_NODES) * s_all, False)
        self.last = None  # (rows, n) of the last resident launch, for post_lists / pack_lists

    # ---- configuration of a context from a model (the fresh-context side, and the warm state)
    @staticmethod
    def configure(env, m):
        env.setMap(m.origin, m.map_dim, m.cells, m.res)
        env.set_control(m.control)
        env.set_u(m.U)
        for k in SM.PARAM_KEYS:
            getattr(env, "set_" + k)(m.params[k])
        env.set_potential_map(m.potential)
        env.set_search_region(m.region)
        Driver.send_goal(env, m.goal)

    @staticmethod
    def send_goal(env, g):
        if g is None:
            env.set_goal(None)
        else:
            env.set_goal(g["row"], w=g["w"], v_max=g["v_max"], tol_pos=g["tol_pos"], tol_vel=g["tol_vel"],
                         tol_acc=g["tol_acc"], tol_yaw=g["tol_yaw"])

    def close(self):
        if not self.light:
            for r in (self.small_rows, self.big_rows, self.lean_rows):
                if r is not None:
                    r.free()
            self.fr.free()
        self.env.close()

    # ---- operations
    def apply(self, op, after):
        """Send `op` to the context; `after` is the model it should then equal."""
        env, c = self.env, op.call
        name = c[0]
        if name == "setMap":
            env.setMap(c[1], c[2], c[3], c[4])
        elif name == "editMap":
            env.editMap(c[1], c[2])
        elif name == "dilate":
            assert np.array_equal(env.dilate(c[1]), after.cells), "dilate: returned map"
        elif name == "freeUnknown":
            assert np.array_equal(env.freeUnknown(), after.cells), "freeUnknown: returned map"
        elif name == "freeAll":
            assert np.array_equal(env.freeAll(), after.cells), "freeAll: returned map"
        elif name == "set_potential_map":
            env.set_potential_map(c[1])
        elif name == "updatePotentialMap":
            assert np.array_equal(env.updatePotentialMap(c[1], c[2], c[3], c[4]), after.cells), "updatePotentialMap: returned map"
        elif name == "set_search_region":
            env.set_search_region(c[1])
        elif name == "setSearchRegion":
            assert np.array_equal(env.setSearchRegion(c[1], c[2], c[3]), after.region), "setSearchRegion: returned region"
        elif name == "set_param":
            getattr(env, "set_" + c[1])(c[2])
        elif name == "set_control":
            env.set_control(c[1])
        elif name == "set_u":
            env.set_u(c[1])
        elif name == "set_goal":
            self.send_goal(env, c[1])
        else:
            self.neutral(op)
        had_goal = self.model.goal is not None
        self.model = after.copy()
        if name == "set_goal" and c[1] is None and had_goal and not self.light:
            with pytest.raises(self._abi.MplxError) as e:  # include/mplx.h: rows that need a goal, without one
                env.expand_lists_resident(self.fr, self.small_rows.arm(_round32(after.nU), True), SM.N_RES)
            assert e.value.code == self._abi.ERR_STATE

    def neutral(self, op):
        """Operations that must change nothing the observers see."""
        env, m, kind = self.env, self.model, op.call[0]
        if kind == "route":
            r = op.call[1]
            env.set_lists_route(r)
            try:  # a forced TILE / GRID route refuses the configurations its kernel does not cover (ERR_STATE)
                self.launch(self.small_rows, SM.N_RES, m.nU, self.reference(), "forced route %s" % r)
            except self._abi.MplxError as e:
                assert r in ("tile", "grid") and e.code == self._abi.ERR_STATE, (r, str(e))
            self.route = r if r in ("auto", "dense") else "auto"  # (the forced kernels do not stay: a later setter may leave their scope)
            env.set_lists_route(self.route)
        elif kind == "service":
            env.service(op.call[1])
            self.service_on = bool(op.call[1])
        elif kind == "read_cells":
            self.check_cells()
        elif kind == "clouds":
            for k, fn in enumerate((env.getCloud, env.getFreeCloud, env.getUnknownCloud)):
                assert np.array_equal(fn(), np_cloud(m.cells, m.map_dim, m.origin, m.res, k)[0]), "cloud %d" % k
        elif kind == "check_edges":
            self.check_edges(self.reference())
        elif kind == "post_lists":
            rows, n = self.last
            goal = np.zeros(env.n_fields)
            goal[:m.dim] = [m.origin[i] + 0.4 * m.map_dim[i] * m.res for i in range(m.dim)]
            got = rows.read(n, m.nU, "before post_lists")
            if "state" not in got:
                return
            rows.n_slots = n * rows.S
            post = env.post_lists(rows, goal, w=7.0, v_max=1.25, tol_pos=0.9, n_nodes=n, want_canon=False)
            got.update(heur=post["heur"][:n * rows.S], flags=post["flags"][:n * rows.S] & 3)
            check_fused_rows(got, goal, m.control, m.dim, 7.0, 1.25, (0.9, -1.0, -1.0, -1.0), "post_lists")
        elif kind == "pack_lists":
            rows, n = self.last
            got = rows.read(n, m.nU, "before pack_lists")
            if "state" not in got:
                return
            rows.n_nodes, rows.n_slots = n, n * rows.S
            packed = env.alloc_packed(n)
            total = env.pack_lists(rows, packed, n, want_total=True)
            p, want = packed.download(), self.m.pack_host_lists(got, n)
            packed.free()
            assert total == want["total"] and np.array_equal(p["offs"], want["offs"])
            for k in ("action", "hash"):
                assert np.array_equal(p[k], want[k]), "pack_lists: " + k
            assert np.array_equal(p["cost"].view(np.uint64), want["cost"].view(np.uint64))
            assert np.array_equal(p["state"].view(np.uint64), want["state"].view(np.uint64))
        elif kind == "synchronize":
            env.synchronize()
        elif kind == "map_upload_bytes":
            a = env.map_upload_bytes()
            assert env.map_upload_bytes() == a
        else:
            raise ValueError(kind)

    # ---- observers
    def reference(self):
        return O.expand(self.model.oracle_env(), self.w.probes, threads=8, ref=self.use_ref)

    def rtol(self):
        return YAW_COST_RTOL if self.model.control & 0x10 else 0.0

    def launch(self, rows, n, S, ref, what):
        m = self.model
        fused = m.goal is not None and "state" in rows.dev
        self.env.expand_lists_resident(self.fr, rows.arm(S, fused), n)
        self.env.synchronize()
        got = rows.read(n, m.nU, what)
        reps = -(-n // SM.N_DISTINCT)
        want = _sub(_tile(ref, reps) if reps > 1 else ref, n, m.nU)
        assert_lists_equal(got, want, n, m.nU, cost_rtol=self.rtol(), what=what)
        if fused:
            g = m.goal
            check_fused_rows(got, np.asarray(g["row"]), g["control"], m.dim, g["w"], g["v_max"],
                             (g["tol_pos"], g["tol_vel"], g["tol_acc"], g["tol_yaw"]), what)
        self.last = (rows, n)
        return got

    def host_batch(self, nodes, ref, what):
        """mplx_expand_lists into poisoned numpy arrays at S = nU: the lists, and nothing past count[k]."""
        m = self.model
        n, nU, F = nodes.shape[1], m.nU, self.env.n_fields
        out = {"stride": nU, "count": _poisoned(np.int32, n), "action": _poisoned(np.int32, n * nU),
               "cost": _poisoned(np.float64, n * nU), "hash": _poisoned(np.uint64, n * nU),
               "state": _poisoned(np.float64, (F, n * nU)), "iters": _poisoned(np.int32, n * nU)}
        got = self.env.expand_lists(nodes, out=out)
        assert ((got["count"] >= 0) & (got["count"] <= nU)).all(), what + ": count"
        past = (np.arange(nU)[None, :] >= got["count"][:, None]).ravel()
        for k in ("action", "cost", "hash", "iters"):
            assert (got[k][past].view(np.uint8) == POISON).all(), "%s: host row `%s` touched past count[k]" % (what, k)
        assert (np.ascontiguousarray(got["state"][:, past]).view(np.uint8) == POISON).all(), what + ": host state rows touched past count[k]"
        assert_lists_equal(got, _sub(ref, n, nU) if n <= SM.N_DISTINCT else _tile(ref, n // SM.N_DISTINCT), n, nU,
                           cost_rtol=self.rtol(), what=what)
        return got

    def get_succ(self, ref, what):
        m, nU = self.model, self.model.nU
        wp = self.m.Waypoint.from_row(m.dim, m.control, self.w.probes[:, 0])
        succ, cost, act = self.env.get_succ(wp)
        st = ref["status"][:nU]
        want = [i for i in range(nU) if st[i] in (1, 2)]
        assert act == want, what + ": get_succ actions"
        for j, i in enumerate(want):
            assert np.array_equal(succ[j].to_row().view(np.uint64), ref["state"][:, i].view(np.uint64)), what + ": get_succ state"
            c = ref["cost"][i]
            assert (np.isinf(cost[j]) and np.isinf(c)) or (abs(cost[j] - c) <= self.rtol() * abs(c)), what + ": get_succ cost"

    def small_calls(self, ref, what):
        """Two host batches in a row and a get_succ: through the resident kernel where the model says it is eligible."""
        m, env = self.model, self.env
        r0 = env.service()
        self.host_batch(self.w.small, ref, what + ", host batch 1")
        self.host_batch(self.w.small, ref, what + ", host batch 2")
        self.get_succ(ref, what)
        r1 = env.service()
        assert r1["failures"] == 0, what
        grew = r1["requests"] - r0["requests"]
        if m.service_eligible() and self.service_on and self.route == "auto":
            if m.nU <= 128:  # (larger tables: whether a workgroup's tile fits the LDS is the library's business)
                assert grew == 2, "%s: expected the second batch and the get_succ to go through the resident kernel, requests grew by %d" % (what, grew)
        else:
            assert grew == 0, "%s: the resident kernel served a configuration outside its scope (%d requests)" % (what, grew)

    def check_mirror(self, what):
        m, env = self.model, self.env
        assert env.has_potential == (m.potential is not None), what + ": EnvMap.has_potential"
        idx = np.arange(min(8, m.n_cells))
        if m.potential is None:
            with pytest.raises(self._abi.MplxError) as e:
                env.read_cells(idx, potential=True)
            assert e.value.code == self._abi.ERR_STATE
        else:
            assert np.array_equal(env.read_cells(idx, potential=True), m.potential[idx]), what + ": potential cells"

    def check_cells(self):
        m, env = self.model, self.env
        idx = np.arange(m.n_cells)
        assert np.array_equal(env.read_cells(idx), m.cells), "map cells differ from the model"
        if m.potential is not None:
            assert np.array_equal(env.read_cells(idx, potential=True), m.potential), "potential cells differ from the model"

    def check_edges(self, ref):
        m = self.model
        if m.control & 0x10 or m.potential is not None:
            return
        nU = m.nU
        st = ref["status"][:SM.N_RES * nU]
        slots = np.nonzero((st == 1) | (st == 2))[0]
        slots = slots[::max(1, slots.size // 300)][:300]
        if slots.size == 0:
            return
        parents = np.ascontiguousarray(self.w.probes[:, slots // nU])
        actions = (slots % nU).astype(np.int32)
        got = self.env.check_edges(parents, actions)
        want = O.check_edges(m.oracle_env(), parents, actions)
        assert np.array_equal(got["free"], want["free"]), "check_edges: free flags"
        assert np.array_equal(got["cost"], want["cost"]), "check_edges: cost"

    def observe(self, what, deep=False):
        m = self.model
        ref = self.reference()
        self.check_mirror(what)
        self.small_calls(ref, what)
        if self.light:
            return ref
        nU = m.nU
        self.launch(self.small_rows, SM.N_RES, nU, ref, what + ", 192 nodes at S = nU")
        if _round32(nU) != nU:
            self.launch(self.small_rows, SM.N_RES, _round32(nU), ref, what + ", 192 nodes at S = 32-multiple")
        rows = self.big_rows if nU <= SM.FULL_ROWS_MAX_NU else self.lean_rows
        self.launch(rows, SM.N_BIG, _round32(nU), ref, what + ", 4096 nodes")
        if deep:
            self.check_cells()
            self.check_edges(ref)
            if nU <= SM.FULL_ROWS_MAX_NU:
                self.host_batch(self.big_nodes, ref, what + ", 4096-node host batch")
        return ref


def _run(engine, plan, deep_every=0):
    d = Driver(engine, plan)
    try:
        d.observe("warm state")
        for j, (op, after, eff) in enumerate(plan.steps):
            try:
                d.apply(op, after)
                last = j == len(plan.steps) - 1
                d.observe("after step %d %r" % (j, op), deep=last or op.kind == "free_unknown" or (deep_every and j % deep_every == deep_every - 1))
            except (AssertionError, d._abi.MplxError) as e:
                raise AssertionError("%s\n  replay: %s" % (e, plan.describe(j + 1))) from e
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ (a) pairwise table
PAIRS = [(s, a, b) for s in SM.SLICES for a, b in SM.pair_kinds(s)]


@pytest.mark.gpu
@pytest.mark.parametrize("slice_name,a,b", PAIRS, ids=["%s-%s>%s" % p for p in PAIRS])
def test_pair_of_mutators_then_the_context_equals_a_fresh_one(engine, oracle_lib, slice_name, a, b):
    _run(engine, SM.pair_plan(slice_name, a, b))


# ------------------------------------------------------------------------------------------------- (b) service table
def _same_lists(a, b, what):
    assert np.array_equal(a["count"], b["count"]), what + ": count"
    used = (np.arange(a["stride"])[None, :] < a["count"][:, None]).ravel()
    for k in ("action", "hash", "iters"):
        assert np.array_equal(a[k][used], b[k][used]), what + ": " + k
    assert np.array_equal(a["cost"][used].view(np.uint64), b["cost"][used].view(np.uint64)), what + ": cost"
    assert np.array_equal(a["state"][:, used].view(np.uint64), b["state"][:, used].view(np.uint64)), what + ": state"


SERVICE_CASES = [(s, k) for s in ("2d_acc", "3d_acc") for k in SM.MUTATORS]


@pytest.mark.gpu
@pytest.mark.parametrize("slice_name,kind", SERVICE_CASES, ids=["%s-%s" % c for c in SERVICE_CASES])
def test_mutator_while_the_service_kernel_is_resident(engine, oracle_lib, slice_name, kind):
    """Resident kernel up, one mutator, two small batches: the oracle's lists for the new state, and the lists of a fresh
    context that never had a resident kernel.  (A mutator that forgets to stop the kernel is answered by the old one.)"""
    plan = SM.service_plan(slice_name, kind)
    op, after, _ = plan.steps[0]
    d = Driver(engine, plan, light=True)
    fresh = engine.EnvMap(d.w.dim, 0)
    try:
        env, b = d.env, d.w.small
        env.expand_lists(b)
        env.expand_lists(b)
        st0 = env.service()
        assert st0["resident"] and st0["requests"] == 1, st0
        d.apply(op, after)
        ref = d.reference()
        g1 = d.host_batch(b, ref, "%r, first batch after it" % op)
        g2 = d.host_batch(b, ref, "%r, second batch after it" % op)
        st1 = env.service()
        assert st1["failures"] == 0
        if after.service_eligible() and after.nU <= 128:
            assert st1["resident"] and st1["requests"] > st0["requests"], (st0, st1)
        d.get_succ(ref, repr(op))
        Driver.configure(fresh, after)
        fresh.service(0)
        f = fresh.expand_lists(b)
        assert fresh.service()["requests"] == 0
        _same_lists(g1, f, "first batch vs a fresh context")
        _same_lists(g2, f, "second batch vs a fresh context")
        d.check_mirror(repr(op))
    finally:
        d.close()  # (first: freeing the other context's buffers would wait for this one's patient kernel to leave)
        fresh.close()


# ---------------------------------------------------------------------------------------------- (c) random sequences
@pytest.mark.gpu
@pytest.mark.parametrize("slice_name,seed,steps,theme", SM.RANDOM_PLANS, ids=["%s-seed%d-%s" % (p[0], p[1], p[3]) for p in SM.RANDOM_PLANS])
def test_random_sequence(engine, oracle_lib, slice_name, seed, steps, theme):
    _run(engine, SM.random_plan(slice_name, seed, steps, theme), deep_every=4)


# ------------------------------------------------------------------------------ the generator, checked without a GPU
NOTICED = ("lists", "fused", "hidden")


class _HostRow:
    def __init__(self, a):
        self.a = a

    def download(self, dtype, shape):
        return self.a.copy()


def _host_rows(S, counts, cap_nodes=6, F=10, spoil=None):
    """Rows over host arrays filled as a correct launch of len(counts) nodes at stride S would leave them."""
    r = Rows.__new__(Rows)
    r.cap_nodes, r.cap_slots, r.F, r.S, r.fused = cap_nodes, cap_nodes * S, F, S, False
    r.names = ["count", "action", "cost", "hash", "state", "iters", "heur", "flags"]
    r.nbytes = {k: (cap_nodes if k == "count" else r.cap_slots * (F if k == "state" else 1)) * ITEM[k][1] for k in r.names}
    raw = {k: np.full(r.nbytes[k], POISON, np.uint8) for k in r.names}
    raw["count"].view(np.int32)[:len(counts)] = counts
    for i, c in enumerate(counts):
        for k in ("action", "cost", "hash", "iters"):
            raw[k].view(ITEM[k][0])[i * S:i * S + c] = 7
        raw["state"].view("<f8").reshape(F, r.cap_slots)[:, i * S:i * S + c] = 1.5
    if spoil:
        spoil(raw)
    r.dev = {k: _HostRow(raw[k]) for k in r.names}
    return r


def test_the_canary_catches_a_write_outside_what_a_launch_may_write():
    counts = [3, 0, 25, 7]
    _host_rows(25, counts).read(4, 25, "clean")

    def padded(raw):  # S % 32 == 0: the rest of the list's last 128-byte line, `action` = -1
        raw["action"].view(np.int32)[3:32] = -1
        raw["cost"].view("<f8")[3:16] = 0.0
    _host_rows(32, counts, spoil=padded).read(4, 25, "line padding")
    planted = {
        "past count[k]": (25, lambda raw: raw["cost"].view("<f8").__setitem__(3, 1.0)),
        "past n_nodes in a state row": (25, lambda raw: raw["state"].view("<f8").reshape(10, -1).__setitem__((9, 100), 1.0)),
        "count of a node past n_nodes": (25, lambda raw: raw["count"].view(np.int32).__setitem__(4, 0)),
        "a row that was not asked for": (25, lambda raw: raw["heur"].view("<f8").__setitem__(0, 0.0)),
        "padding that looks like a successor": (32, lambda raw: raw["action"].view(np.int32).__setitem__(3, 5)),
        "padding behind an empty list": (32, lambda raw: raw["iters"].view(np.int32).__setitem__(33, 5)),
        "padding without a 32-multiple stride": (25, lambda raw: raw["action"].view(np.int32).__setitem__(3, -1)),
    }
    for what, (S, spoil) in planted.items():
        with pytest.raises(AssertionError):
            _host_rows(S, counts, spoil=spoil).read(4, 25, what)


def test_pair_table_covers_every_ordered_pair_of_the_alphabet():
    have = {(a, b) for _, a, b in PAIRS}
    assert have == {(a, b) for a in SM.MUTATORS for b in SM.MUTATORS}
    assert {k for _, k in SERVICE_CASES} == set(SM.MUTATORS)
    # every kind has variants, and the variants of the alphabet's setters are all reachable
    for s in SM.SLICES:
        w = SM.world(s)
        for k in SM.MUTATORS:
            assert len(SM.variants(w, w.warm(potential=True), k)) >= 1, (s, k)


@pytest.mark.parametrize("slice_name", list(SM.SLICES))
def test_every_step_of_the_tables_can_be_noticed(oracle_lib, slice_name):
    """A stale context is caught only if the step changes the answer: on the 24-node batch the oracle's lists before and
    after every step differ (for the goal: the heur / flags rows; behind a potential map: equal now, different once it is
    removed) -- or the step is one of those that cannot, by a rule (sequence_model.structural_reason) or by name
    (sequence_model.BY_CHANCE)."""
    plans = [SM.pair_plan(slice_name, a, b) for a, b in SM.pair_kinds(slice_name)]
    if slice_name != "2d_yaw_pot":
        plans += [SM.service_plan(slice_name, k) for k in SM.MUTATORS]
    by_chance = set()
    for p in plans:
        models = p.models()
        for j, (op, after, eff) in enumerate(p.steps):
            before = models[j]
            if before.potential is not None and after.potential is not None and op.kind in SM.OCCUPANCY_OPS \
                    and SM.structural_reason(before, op.kind) is None and eff != "cells":
                assert eff == "hidden", "%s: an occupancy edit behind a potential map must not change the lists (%s)" % (p.describe(j + 1), eff)
            if eff in NOTICED or SM.structural_reason(before, op.kind):
                continue
            assert (slice_name, p.label, j) in SM.BY_CHANCE, "%s: step %d changes nothing an observer sees" % (p.describe(j + 1), j)
            by_chance.add((slice_name, p.label, j))
    assert by_chance == {k for k in SM.BY_CHANCE if k[0] == slice_name}


def test_random_sequences_are_mostly_noticeable_and_reach_every_kind(oracle_lib):
    seen, total, dull = set(), 0, 0
    for args in SM.RANDOM_PLANS:
        for op, _, eff in SM.random_plan(*args).steps:
            if op.kind in SM.MUTATORS:
                total += 1
                dull += eff not in NOTICED
                if eff in NOTICED:
                    seen.add(op.kind)
    assert 5 * dull <= total, (dull, total)
    # freeUnknown cannot change a list (structural_reason): the map read-back after it is its observer
    assert seen == set(SM.MUTATORS) - {"free_unknown"}, set(SM.MUTATORS) - seen
    themes = {a[3] for a in SM.RANDOM_PLANS}
    assert {"geometry", "tables"} <= themes
    for args in SM.RANDOM_PLANS:
        if args[3] == "geometry":
            sizes = [int(np.prod(m.map_dim)) for m in SM.random_plan(*args).models()]
            d = np.sign(np.diff(sizes))
            assert (d > 0).any() and (d < 0).any(), "a geometry sequence grows and shrinks the map"
        if args[3] == "tables":
            assert len({m.nU for m in SM.random_plan(*args).models()}) >= 2


@pytest.mark.skipif(not os.path.exists(O.REF_PLANNER_SO), reason="reference build (oracle/_ref) not present")
@pytest.mark.parametrize("slice_name", ["2d_acc", "3d_acc"])
def test_chained_map_operations_of_the_model_equal_the_reference(slice_name):
    """dilate -> updatePotentialMap -> editMap -> updatePotentialMap (on an already potential-valued map) ->
    setSearchRegion -> dilate -> updatePotentialMap with a range box: after every MapPlanner operation of the chain the
    model holds what the reference's own MapPlanner makes of the model's previous state.  (MapUtil::dilate has no hook in
    the reference build here; its restatement is pinned by tests/golden/map_util_golden.npz and chained as it is.)"""
    w = SM.world(slice_name)
    m = w.base.copy()
    chain = ["dilate", "pot_update", "edit", "pot_update", "region_path", "dilate", "pot_update", "free_unknown", "pot_update"]
    n_prep = 0
    for j, kind in enumerate(chain):
        op = SM.variants(w, m, kind)[j % len(SM.variants(w, m, kind))]
        before = m.copy()
        SM.apply_to_model(m, op)
        c = op.call
        if c[0] == "updatePotentialMap":
            want = O.update_potential_map(before.cells, before.map_dim, before.origin, before.res, c[1], c[2], c[3], c[4], ref=True)
            assert np.array_equal(m.cells, want) and np.array_equal(m.potential, want), (j, op)
            assert not np.array_equal(before.cells, m.cells)
            n_prep += 1
        elif c[0] == "setSearchRegion":
            want = O.search_region(before.map_dim, before.origin, before.res, c[1], c[2], c[3], ref=True)
            assert np.array_equal(m.region, want) and 0 < want.sum() < want.size, (j, op)
            n_prep += 1
        elif c[0] == "dilate":
            assert np.array_equal(m.cells, np_dilate(before.cells, before.map_dim, c[1]))
    assert n_prep == 5
    assert ((m.cells > 0) & (m.cells < 100)).any(), "the chain ends on a potential-valued map"
