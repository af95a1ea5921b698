"""GPU: include/mplx_prior.h against tests/prior_model.py where tests/test_gpu_prior.py does not go, bit for bit: the
prior table in 2D and 3D for every prior control (VEL .. SNP, each with and without the yaw bit) under a prior dt that is
no multiple of the context's (and under two pairs at which the segment guess of find_segment needs correcting), 65 priors
a call of lengths 1 .. 12 with the hand-made ones of tests/prior_orders_cases.py among them; 1, 63, 64 and 257 queries,
one shared start, the 4- and the 16-lane traverse, the raw call with padded strides and a second call that reuses the buffers; every push in 3D (open, closed, with the ray trace) at accumulated times and for
67 interleaved queries; the two-stage search in 3D round for round, with best= and through a replan; and an ACC prior
for a 2D JRK search of one query.  The conditions on the inputs are checked on the model (tests/test_prior_orders.py runs
the same checks without a GPU) before the device is asked."""
import ctypes as C
import math

import numpy as np
import pytest

import multi_model as MM
import open_best_model as BM
import open_model as OM
import prior_model as PM
import prior_orders_cases as PC
import replan_model as RM
from table_model import TableModel, oracle_provider
from test_gpu_multi import assert_multi_table_equal
from test_gpu_open import assert_open_equal, assert_result_equal
from test_gpu_prior import assert_prior_equal
from test_gpu_table import assert_table_equal, bits

pytestmark = pytest.mark.gpu


def make_env(m, D, dt, v_max=PC.VMAX, with_pot=True):
    cells, pot = PC.world(D)
    env = m.EnvMap(D)
    env.setMap(PC.ORIGIN[D], PC.DIMS[D], cells, PC.RES)
    if with_pot:
        env.set_potential_map(pot)
    env.set_control(PC.SEARCHING[D])
    env.set_u(PC.prior_u(D, PC.SEARCHING[D], 0.5))
    env.set_v_max(v_max)
    env.set_a_max(1.0)
    env.set_dt(dt)
    env.set_w(PC.W)
    env.set_potential_weight(PC.POT_W)
    env.set_gradient_weight(PC.GRAD_W)
    return env


def open_set(env, goals, capacity=512):
    tab = env.alloc_table(capacity, n_queries=goals.shape[0])
    opn = env.alloc_open(tab)
    opn.set_goals(goals, tol_pos=0.5)
    return tab, opn


def assert_tables_equal(info, got, want, what=""):
    assert got is not None, what
    if info is not None:
        assert info["status"].tolist() == [w["status"] for w in want], what
        assert info["n_steps"].tolist() == [w["n_steps"] for w in want], what
    assert got["n_steps"].tolist() == [w["n_steps"] for w in want], what
    for q, w in enumerate(want):
        assert_prior_equal(got, q, w, "%s: query %d" % (what, q))


def close(env, *pairs):
    for tab, opn in pairs:
        opn.free()
        tab.free()
    env.close()


# ---- 1. the table ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", PC.TABLE_CASES, ids=PC.table_id)
def test_table_in_every_dimension_for_every_prior_control(engine, case):
    m = engine
    D, name, pdt, dt = case
    print(PC.table_id(case), PC.check_table_case(case))  # the conditions on the inputs, on the model
    starts, actions, U, goals, want = PC.table_case(case)
    env = make_env(m, D, dt)
    tab, opn = open_set(env, goals)
    assert opn.priors() is None
    info = opn.set_priors(starts, actions, PC.CONTROLS[name], U, pdt)
    assert_tables_equal(info, opn.priors(), want, PC.table_id(case))
    close(env, (tab, opn))


@pytest.mark.parametrize("Q", PC.QUERY_COUNTS)
def test_table_of_1_63_64_and_257_queries(engine, Q):
    """set_prior_list, one entry None at an interior position: past one wave and one past a block of prior_build_kernel."""
    m = engine
    starts, actions, U, goals, none, want = PC.count_case(Q)
    priors = []
    for q in range(Q):
        acts = actions[:, q]
        n = int(np.argmax(acts == -1)) if np.any(acts == -1) else acts.size
        priors.append(None if q == none else m.search.Prior(starts[:, q], acts[:n], PC.ACC, U, 0.3))
    env = make_env(m, 3, 0.1)
    tab, opn = open_set(env, goals)
    info = opn.set_prior_list(priors)
    assert_tables_equal(info, opn.priors(), want, "Q = %d" % Q)
    close(env, (tab, opn))


def test_table_of_64_priors_from_one_shared_start(engine):
    m = engine
    starts, actions, U, goals, want = PC.shared_start_case()
    env = make_env(m, 3, 0.1)
    tab, opn = open_set(env, goals)
    info = opn.set_priors(starts[:, 0], actions, PC.ACC, U, 0.3)
    assert_tables_equal(info, opn.priors(), want, "n_starts == 1")
    close(env, (tab, opn))


def test_table_through_the_16_lane_traverse(engine):
    """B = ceil(v_max * horizon * dt_prior / res) + 1 in (64, 256] (the table cases have B <= 64, the corridor of
    tests/test_gpu_prior.py B > 256): the classes are asserted from the formula, so a changed default is noticed."""
    m = engine
    assert PC.traverse_class(PC.LANES16_VMAX, PC.H_TABLE, 0.3, PC.RES) == (16, 88)
    assert PC.traverse_class(PC.VMAX, PC.H_TABLE, 0.3, PC.RES)[0] == 4 and PC.traverse_class(1.0, 40, 1.0, 0.05)[0] == 64
    starts, actions, U, goals, want = PC.lanes16_case()
    env = make_env(m, 3, 0.1, v_max=PC.LANES16_VMAX)
    tab, opn = open_set(env, goals)
    info = opn.set_priors(starts, actions, PC.JRK, U, 0.3)
    assert_tables_equal(info, opn.priors(), want, "16 lanes")
    close(env, (tab, opn))


def test_raw_call_with_padded_strides_and_reused_buffers(engine):
    """mplx_open_set_priors_device with start_stride > n_starts and action_stride > n_traj, the padding filled with a
    pattern: the table of the packed call.  Then a shorter horizon on the same open set, whose buffers are reused with
    another step capacity: the bytes a fresh open set gives."""
    m = engine
    L_ = m._abi.lib()
    case = (3, "ACC", 0.3, 0.1)
    starts, actions, U, goals, want = PC.table_case(case)
    F, Q = starts.shape
    H = actions.shape[0]
    ss, as_ = Q + 7, Q + 5
    ps = np.full((F, ss), 1e30)
    ps[:, :Q] = starts
    pa = np.full((H, as_), 0x5a5a5a5a, np.int32)
    pa[:, :Q] = actions
    env = make_env(m, 3, 0.1)
    tab, opn = open_set(env, goals)
    d_s, d_a, d_U = m.DeviceArray(env, ps.nbytes), m.DeviceArray(env, pa.nbytes), m.DeviceArray(env, U.nbytes)
    d_s.upload(ps)
    d_a.upload(pa)
    d_U.upload(np.ascontiguousarray(U))

    def call(o, horizon):
        s = m._abi.TrajSet()
        s.starts, s.n_starts, s.start_stride, s.actions = d_s.ptr, Q, ss, d_a.ptr
        s.n_traj, s.horizon, s.action_stride = Q, horizon, as_
        p = m._abi.PriorSource()
        p.control, p.nU, p.udim, p.U, p.dt = PC.ACC, U.shape[0], U.shape[1], d_U.ptr, 0.3
        status, n_steps = np.zeros(Q, np.uint8), np.zeros(Q, np.int32)
        info = m._abi.PriorInfo()
        info.status, info.n_steps = status.ctypes.data, n_steps.ctypes.data
        assert L_.mplx_open_set_priors_device(o._open, C.byref(p), C.byref(s), C.byref(info)) == m._abi.OK
        return {"status": status, "n_steps": n_steps}
    env._flush()
    info = call(opn, H)
    assert_tables_equal(info, opn.priors(), want, "padded strides")
    # a shorter horizon: every prior cut to 5 actions (the bad action of query 1 is at 4, the empty prior stays empty)
    short = PC.model_tables(3, PC.ACC, 0.3, 0.1, starts, actions[:5], U, goals)
    assert max(w["n_steps"] for w in short) < max(w["n_steps"] for w in want)
    info = call(opn, 5)
    got = opn.priors()
    assert_tables_equal(info, got, short, "shorter horizon, buffers reused")
    tab2, opn2 = open_set(env, goals)
    opn2.set_priors(starts, actions[:5], PC.ACC, U, 0.3)
    fresh = opn2.priors()
    for q in range(Q):
        for k in ("pos", "togo", "goal_row"):
            assert np.array_equal(bits(got[k][q]), bits(fresh[k][q])), (k, q)
    assert np.array_equal(got["n_steps"], fresh["n_steps"]) and np.array_equal(got["goal_hash"], fresh["goal_hash"])
    for b in (d_s, d_a, d_U):
        b.free()
    close(env, (tab, opn), (tab2, opn2))


# ---- 2. the push in 3D -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["three", "many"])
def test_push_with_priors_in_3d(engine, oracle_lib, which):
    """open_push_kernel<3, true, {false, true}, true>: the open push, the closed push and the push with the ray trace on
    the cases of tests/prior_orders_cases.py::push_case -- "three": the case list of test_gpu_prior.py::test_push_with_priors
    at context dt 0.1 with accumulated times; "many": 67 interleaved queries, 335 rows, priors of 6 .. 36 steps."""
    m, O = engine, oracle_lib
    case = PC.push_case(which)
    goals, starts, actions, U, pri, states, query, g = case
    table, want_fr, model, plain, counts = PC.check_push_case(O, case, MM)  # the prior moves keys, and only its queries'
    print(which, counts)
    Q, n = goals.shape[0], states.shape[1]
    env = make_env(m, 3, PC.PUSH_DT, with_pot=False)
    tab, opn = open_set(env, goals, capacity=1024)
    info = opn.set_priors(starts, actions, PC.ACC, U, PC.PUSH_PDT)
    assert info["n_steps"].tolist() == [p["n_steps"] if p else 0 for p in pri]
    fr = m.TableFrontier(env, n)
    count = tab.seed(states, g, frontier=fr, query=query)
    assert count == want_fr["count"] == n
    assert_multi_table_equal(tab, table)
    opn.push(fr, n_max=count, eps=1.0)
    model.push(want_fr, count, 1.0)
    assert_open_equal(opn, model, "open push")
    opn.clear()
    model.f, model.flags = {}, {}
    opn.push(fr, n_max=count, eps=2.0, closed=True)
    RM.push_closed(model, want_fr, count, 2.0)
    assert_open_equal(opn, model, "closed push")
    opn.clear()
    model.f, model.flags = {}, {}
    opn.push(fr, n_max=count, eps=1.0, sight=True)
    model.push(want_fr, count, 1.0, sight=1)
    assert_open_equal(opn, model, "push with sight")
    opn.clear_priors()
    opn.clear()
    opn.push(fr, n_max=count, eps=1.0)
    plain.f, plain.flags = {}, {}
    plain.push(want_fr, count, 1.0)
    assert_open_equal(opn, plain, "after clear_priors")
    fr.free()
    close(env, (tab, opn))


# ---- 3. the search -----------------------------------------------------------------------------------------------------------

class PriorBestModel(PM.PriorMultiOpenModel, BM.MultiOpenBestModel):
    """The keys of the prior model under the selection rule of the best-k model: the two classes composed, neither restated."""
    best = 16

    def select_many(self, delta, capacity):
        return self.select_best_many(self.best, delta, capacity)


def s3_env(m, control):
    env = m.EnvMap(3)
    env.setMap(PC.S3_ORIGIN, PC.S3_DIMS, PC.s3_cells(), PC.S3_RES)
    env.set_control(control)
    env.set_u(PC.s3_u())
    env.set_v_max(PC.S_VMAX)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    env.set_w(PC.S_W)
    return env


def s3_first_stage(m, O):
    """search_many at VEL on the device, equal to the model's stage, and its paths as priors with one replaced by None."""
    S, acts, pri, out1 = PC.s3_priors(O, MM)
    env1 = s3_env(m, PC.VEL)
    r1 = env1.search_many(S, PC.rows_of(PC.S3_GOALS, 14), eps=1.0, delta=0.0, g_max=PC.S3_GMAX, capacity=1 << 12, sight=False)
    assert r1.status == out1["status"] == [OM.FOUND] * 3 and (r1.rounds, r1.expanded) == (out1["rounds"], out1["expanded"])
    priors = r1.as_priors()
    for q in range(3):
        assert priors[q].actions.tolist() == acts[q] and np.array_equal(bits(priors[q].start), bits(S[:, q])), q
        assert priors[q].control == PC.VEL and priors[q].dt == 1.0 and np.array_equal(priors[q].U, PC.s3_u())
    priors[PC.S3_NONE] = None
    r1.free()
    env1.close()
    return S, priors, pri


@pytest.mark.parametrize("delta", [0.0, 10.0])
def test_two_stage_search_in_3d(engine, oracle_lib, delta):
    m, O = engine, oracle_lib
    _, _, plain, _ = PC.s3_stage(O, MM, PC.ACC, [None] * 3, delta)
    S, priors, pri = s3_first_stage(m, O)
    table, model, want, _ = PC.s3_stage(O, MM, PC.ACC, pri, delta)
    for q in range(3):  # a guided query expands fewer nodes than the same query unguided
        assert q == PC.S3_NONE or 2 * want["expanded"][q] < plain["expanded"][q]
    env = s3_env(m, PC.ACC)
    r2 = env.search_many(S, PC.rows_of(PC.S3_GOALS, 14), eps=1.0, delta=delta, g_max=PC.S3_GMAX, capacity=1 << 16, sight=False,
                         priors=priors)
    print(delta, r2, r2.rounds, r2.expanded, r2.cost, plain["expanded"])
    assert r2.status == want["status"] == [OM.FOUND] * 3 and want["truncated"] == 0
    assert (r2.rounds, r2.expanded, r2.total_rounds) == (want["rounds"], want["expanded"], want["total_rounds"])
    for q in range(3):
        assert_result_equal(r2.last_select[q], want["results"][q], "query %d" % q)
    got = r2.open.priors()
    for q in range(3):
        if pri[q] is not None:
            assert_prior_equal(got, q, pri[q], "query %d" % q)
    assert got["n_steps"][PC.S3_NONE] == 0
    assert_multi_table_equal(r2.table, table)
    assert_open_equal(r2.open, model)
    r2.free()
    env.close()


def test_best_with_priors_and_a_replan_that_keeps_both(engine, oracle_lib):
    m, O = engine, oracle_lib
    S, priors, pri = s3_first_stage(m, O)
    table, model, want, _ = PC.s3_stage(O, MM, PC.ACC, pri, math.inf, model_class=PriorBestModel, best=16)
    assert want["status"] == [OM.FOUND] * 3 and max(h["count"] for hq in want["history"] for h in hq) == 16
    env = s3_env(m, PC.ACC)
    G = PC.rows_of(PC.S3_GOALS, 14)
    r2 = env.search_many(S, G, eps=1.0, delta=math.inf, g_max=PC.S3_GMAX, capacity=1 << 16, sight=False, priors=priors, best=16)
    print(r2, r2.rounds, r2.expanded, r2.cost)
    assert r2.status == want["status"]
    assert (r2.rounds, r2.expanded, r2.total_rounds) == (want["rounds"], want["expanded"], want["total_rounds"])
    for q in range(3):
        assert_result_equal(r2.last_select[q], want["results"][q], "query %d" % q)
    got = r2.open.priors()
    for q in range(3):
        if pri[q] is not None:
            assert_prior_equal(got, q, pri[q], "query %d" % q)
    assert_multi_table_equal(r2.table, table)
    assert_open_equal(r2.open, model)
    # replan(advance=2): the open set keeps the priors, the result keeps best
    d0 = r2.table.download()
    roots = [int(r2.table.path(r2.goal_id[q])[0][2]) for q in range(3)]
    n_steps = r2.open.priors()["n_steps"].tolist()
    t = RM.table_from_arrays(d0, n_queries=3)
    mo = PriorBestModel(t, 3, G, [O.lattice_hash(3, PC.ACC, g) for g in G], PC.S_W, PC.S_VMAX, 1.0, pri, tol_pos=0.5)
    oenv = O.Env(3, PC.ACC, PC.s3_u(), PC.s3_cells(), PC.S3_DIMS, PC.S3_ORIGIN, PC.S3_RES, v_max=PC.S_VMAX, a_max=1.0, dt=1.0)
    want3 = RM.replan(t, mo, oracle_provider(O, oenv), RM.OracleEdges(O, oenv, t), 27, 1.0, math.inf, 48, roots=roots,
                      g_max=PC.S3_GMAX)
    r3 = r2.replan(advance=2)
    print(r3, r3.rebase_info, want3["info"], want3["rounds"], want3["expanded"])
    assert r3.open.priors() is not None and r3.open.priors()["n_steps"].tolist() == n_steps and n_steps[PC.S3_NONE] == 0
    assert r3.status == want3["status"] == [OM.FOUND] * 3
    assert (r3.rebase_info["n_kept"], r3.rebase_info["n_roots"]) == (want3["info"]["n_kept"], 3)
    assert (r3.rounds, r3.expanded, r3.total_rounds) == (want3["rounds"], want3["expanded"], want3["total_rounds"])
    for q in range(3):
        assert_result_equal(r3.last_select[q], want3["results"][q], "query %d" % q)
    assert_multi_table_equal(r3.table, t)
    assert_open_equal(r3.open, mo)
    r3.free()
    env.close()


def test_acc_prior_for_a_jrk_search_of_one_query_in_2d(engine, oracle_lib):
    """env.search(prior=Prior(...)) with prior dt 0.5 under dt 0.25: the single-query path through the open set's own
    goals, against PriorOpenModel."""
    m, O = engine, oracle_lib
    cells, U1, U2, start, goal, acts, pri = PC.s2_case()
    env = m.EnvMap(2)
    env.setMap(PC.S2_ORIGIN, PC.S2_DIMS, cells, PC.S2_RES)
    env.set_control(PC.JRK)
    env.set_u(U2)
    env.set_v_max(PC.S_VMAX)
    env.set_a_max(2.0)
    env.set_dt(PC.S2_DT)
    env.set_w(PC.S_W)
    oenv = O.Env(2, PC.JRK, U2, cells, PC.S2_DIMS, PC.S2_ORIGIN, PC.S2_RES, v_max=PC.S_VMAX, a_max=2.0, dt=PC.S2_DT)
    outs = []
    for p in (None, pri):
        table = TableModel(10)
        model = PM.PriorOpenModel(table, 2, goal, O.lattice_hash(2, PC.JRK, goal), PC.S_W, PC.S_VMAX, PC.S2_DT, prior=p, tol_pos=0.5)
        want = OM.search(table, model, oracle_provider(O, oenv), start, O.lattice_hash(2, PC.JRK, start), 1.0, 2.5, 1 << 14)
        outs.append((table, model, want))
    table, model, want = outs[1]
    assert want["status"] == OM.FOUND and outs[0][0].n_nodes != table.n_nodes  # the prior changes what the search does
    r = env.search(start, goal, eps=1.0, delta=2.5, capacity=1 << 14, sight=False,
                   prior=m.search.Prior(start, acts, PC.ACC, U1, PC.S2_PDT))
    print(r, r.last_select, want["rounds"], want["expanded"], table.n_nodes)
    assert r.status == want["status"] and (r.rounds, r.expanded) == (want["rounds"], want["expanded"])
    assert_result_equal(r.last_select, want["result"])
    assert_prior_equal(r.open.priors(), 0, pri)
    assert_table_equal(r.table, table)
    assert_open_equal(r.open, model)
    r.free()
    env.close()
