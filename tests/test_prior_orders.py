"""CPU: the generic part of tests/prior_model.py (dimension, order, yaw) held to second statements, and the conditions
the inputs of tests/test_gpu_prior_orders.py must satisfy, checked on the model alone (tests/prior_orders_cases.py).

The model's table equals the host planner's (mplx_planner_prior_table) bit for bit in 3D for VEL and ACC first planners
under a JRK second planner, without and with a potential map, and in 2D for an ACC first planner.  For the orders a host
first stage is impractical for (JRK, SNP, the yaw flags) the model's chain is held to the oracle's successor instead: the
state after each action of a random sequence is the oracle's successor state for that (state, control), every row, in 2D
and 3D.  The lattice hash equals the oracle's for all 16 (dim, control) pairs.  No GPU."""
import itertools

import numpy as np
import pytest

import multi_model as MM
import prior_model as PM
import prior_orders_cases as PC
from oracle import oracle as O
from test_prior import _planner, assert_same_table, bits, host_table

DIM_CONTROL = [(D, name) for D in (2, 3) for name in PC.CONTROLS]


# ---- the lattice hash and the chain against the oracle -----------------------------------------------------------------------

@pytest.mark.parametrize("D, name", DIM_CONTROL)
def test_lattice_hash_is_the_oracles(oracle_lib, D, name):
    control = PC.CONTROLS[name]
    rng = np.random.default_rng(D * 100 + control)
    rows = rng.uniform(-20.0, 20.0, (200, 4 * D + 2))
    rows[:40] = np.round(rows[:40] * 20.0) / 20.0  # halves of the quantisation steps: the ties of std::round
    seen = set()
    for r in rows:
        h = PM.lattice_hash(D, control, r)
        assert h == oracle_lib.lattice_hash(D, control, r)
        seen.add(h)
    assert len(seen) == 200


@pytest.mark.parametrize("pdt", [0.3, 0.5])
@pytest.mark.parametrize("D, name", DIM_CONTROL)
def test_chain_is_the_oracles_successor(oracle_lib, D, name, pdt):
    """_coeffs and _waypoint, which is all the orders above VEL add to the model: the chain of prior_table, one action at
    a time, against the end state of the oracle's successor on an empty map without limits."""
    control = PC.CONTROLS[name]
    K, F = PM._order(control), 4 * D + 2
    U = PC.prior_u(D, control)
    rng = np.random.default_rng(7 * D + control)
    dims = PC.DIMS[D]
    oenv = oracle_lib.Env(D, control, U, np.zeros(int(np.prod(dims)), np.int8), dims, [-1000.0] * D, 100.0, dt=pdt)
    compared = 0
    for trial in range(3):
        s = np.zeros(F)
        s[:D] = rng.uniform(-3.0, 3.0, D)
        for k in range(1, K):  # the derivative rows the order reads are live
            s[k * D:(k + 1) * D] = rng.uniform(-0.8, 0.8, D)
        if control & PC.YAW:
            s[4 * D] = rng.uniform(-3.0, 3.0)
        s = [float(x) for x in s]
        for a in rng.integers(0, U.shape[0], 12):
            u = [float(x) for x in U[a]]
            cs = PM._coeffs(D, K, s, u)
            nxt = PM._waypoint(D, control, cs, s, u, pdt)
            nxt[4 * D + 1] = s[4 * D + 1] + pdt
            d = oracle_lib.expand(oenv, np.array(s).reshape(F, 1))
            if d["status"][a] == 0:  # the successor stays in its lattice state: the oracle emits none to compare with
                assert PM.lattice_hash(D, control, nxt) == PM.lattice_hash(D, control, s), (name, trial, a)
                s = nxt
                continue
            compared += 1
            assert d["status"][a] in (1, 2), (name, trial, a, d["status"][a])
            got = d["state"][:, a]
            rows = F if control & PC.YAW else 4 * D  # (the yaw row of a control without the yaw bit is not the model's)
            assert np.array_equal(bits(np.array(nxt)[:rows] + 0.0), bits(got[:rows] + 0.0)), (name, trial, a, nxt, got)
            assert bits([nxt[4 * D + 1]])[0] == bits([got[4 * D + 1]])[0]
            s = nxt
    assert compared >= 30


# ---- the model's table against the host planner's, beyond 2D VEL -------------------------------------------------------------

H3 = {"dim": [13, 11, 9], "origin": [-3.3, -2.7, -2.2], "res": 0.5}
H2 = {"dim": [19, 13], "origin": [-4.8, -3.2], "res": 0.5}


def host_world(D):
    """A small non-cube map with a slab the plan has to go around, and a hand-made potential map on it."""
    c = dict(H3 if D == 3 else H2)
    dims = c["dim"]
    grid = np.zeros(dims[::-1], np.int8)
    if D == 3:
        grid[2:, 3:, 6] = 100
    else:
        grid[4:, 9] = 100
    cells = grid.ravel()
    rng = np.random.default_rng(50 + D)
    pot = rng.integers(0, 60, cells.size).astype(np.int8)
    pot[cells == 100] = 100
    c["cells"], c["pot"] = cells, pot
    lo = [c["origin"][i] + 1.5 * c["res"] for i in range(D)]
    hi = [c["origin"][i] + (dims[i] - 1.5) * c["res"] for i in range(D)]
    c["start"], c["goal"] = np.array(lo), np.array([hi[0]] + lo[1:]) if D == 3 else np.array([hi[0], lo[1]])
    return c


_first = {}


def first_plan(m, D, name):
    """The first planner's plan on the oracle provider: (planner, start row, actions, U, keep)."""
    if (D, name) not in _first:
        c, keep = host_world(D), []
        control = PC.CONTROLS[name]
        U = np.array(list(itertools.product([-1.0, 0.0, 1.0], repeat=D)))
        first = _planner(m, c, control, U, c["cells"], 1.0, keep, dim=D)
        ok = first.plan(m.Waypoint(D, control, pos=c["start"]), m.Waypoint(D, control, pos=c["goal"]))
        assert ok, (D, name)
        tr = first.getTraj()
        _first[(D, name)] = (first, np.array(tr.nodes[0]), np.array(tr.actions, dtype=np.int32), U, keep)
    return _first[(D, name)]


@pytest.mark.parametrize("potential, gradient_weight", [(False, 0.0), (True, 0.0), (True, 0.25)])
@pytest.mark.parametrize("D, name", [(3, "VEL"), (3, "ACC"), (2, "ACC")])
def test_the_model_table_is_the_host_planners_beyond_2d_vel(engine, D, name, potential, gradient_weight):
    m = engine
    c, keep = host_world(D), []
    first, start, actions, U1, _ = first_plan(m, D, name)
    assert len(actions) >= 5
    U = 0.5 * U1
    pot = c["pot"] if potential else None
    second = _planner(m, c, m.JRK, U, pot if potential else c["cells"], 0.5, keep, dim=D)
    second.setW(10)
    if potential:
        second.setPriorTrajectory(first, potential=pot, potential_weight=0.5, gradient_weight=gradient_weight)
    else:
        second.setPriorTrajectory(first)
    host = host_table(m, second, dim=D)
    second.close()
    model = PM.prior_table(D, PC.CONTROLS[name], U1, 1.0, start, actions, c["cells"], c["dim"], c["origin"], c["res"], 1.0, 10.0, 0.5,
                           pot=pot, pot_w=0.5, grad_w=gradient_weight)
    assert host["control"] == PC.CONTROLS[name] and host["n_steps"] == 2 * len(actions)
    assert_same_table(model, host, (D, name, potential, gradient_weight))
    assert np.all(np.isfinite(model["togo"]))
    if potential:
        plain = PM.prior_table(D, PC.CONTROLS[name], U1, 1.0, start, actions, c["cells"], c["dim"], c["origin"], c["res"], 1.0, 10.0, 0.5)
        assert not np.array_equal(model["togo"], plain["togo"])
    assert model["goal_hash"] == O.lattice_hash(D, PC.CONTROLS[name], model["goal_row"])


# ---- the conditions on the inputs of the GPU tests, on the model alone -------------------------------------------------------

@pytest.mark.parametrize("case", PC.TABLE_CASES, ids=PC.table_id)
def test_table_cases_are_not_vacuous(case):
    print(PC.table_id(case), PC.check_table_case(case))


def test_every_dim_and_control_is_a_table_case():
    assert {(c[0], c[1]) for c in PC.TABLE_CASES} == set(DIM_CONTROL)


def test_further_table_cases_are_what_they_say():
    for Q in PC.QUERY_COUNTS:
        starts, actions, U, goals, none, want = PC.count_case(Q)
        assert len(want) == Q and (Q == 1 or (0 < none < Q - 1 and want[none]["n_steps"] == 0))
        assert sum(1 for w in want if w["n_steps"] > 0) >= max(1, (2 * Q) // 3)
    assert 257 in PC.QUERY_COUNTS and 257 > 256  # one past a block of prior_build_kernel
    starts, actions, U, goals, want = PC.shared_start_case()
    assert starts.shape[1] == 1 and len({w["n_steps"] for w in want}) >= 6
    starts, actions, U, goals, want = PC.lanes16_case()
    m = PC.measure(3, want, 0.1)
    assert PC.traverse_class(PC.LANES16_VMAX, PC.H_TABLE, 0.3, PC.RES) == (16, 88)
    assert PC.traverse_class(PC.VMAX, PC.H_TABLE, 0.3, PC.RES) == (4, 30) and PC.traverse_class(PC.VMAX, PC.H_TABLE, 0.5, PC.RES) == (4, 49)
    assert PC.traverse_class(1.0, 40, 1.0, 0.05) == (64, 801)  # the corridor of tests/test_gpu_prior.py
    assert 4 * m["finite"] >= m["non_empty"] and 10 * m["infinite"] >= m["non_empty"] and m["skipped"] >= 1, m
    assert max(len(w.get("samples", [])) for w in want) > 64  # more samples than one round of 16 lanes, and than one wave


@pytest.mark.parametrize("which", ["three", "many"])
def test_push_cases_are_not_vacuous(oracle_lib, which):
    case = PC.push_case(which)
    table, fr, model, plain, n = PC.check_push_case(oracle_lib, case, MM)
    print(which, n)
    pri, query = case[4], case[6]
    if which == "three":
        assert [p is not None for p in pri] == [True, False, True] and n["goal_bits"] >= 6
    else:
        assert n["rows"] >= 300 and len(pri) == 67 and sum(p is None for p in pri) >= 9
        assert len({p["n_steps"] for p in pri if p}) >= 6 and n["inf_keys"] >= 5
        assert np.array_equal(query[:67], np.arange(67))  # interleaved: one wave reads the tables of 64 queries


def test_search_cases_are_not_vacuous(oracle_lib):
    """The 3D world shows something: the VEL stage finds every goal, and a guided query of the ACC stage expands fewer
    nodes than the same query unguided; the query without a prior does what it does unguided."""
    S, acts, pri, out1 = PC.s3_priors(oracle_lib, MM)
    assert out1["status"] == [1, 1, 1] and all(len(a) >= 6 for a in acts)
    for delta in (0.0, 10.0):
        _, _, plain, _ = PC.s3_stage(oracle_lib, MM, PC.ACC, [None] * 3, delta)
        _, _, guided, _ = PC.s3_stage(oracle_lib, MM, PC.ACC, pri, delta)
        print(delta, plain["expanded"], guided["expanded"], plain["total_rounds"], guided["total_rounds"])
        assert plain["status"] == guided["status"] == [1, 1, 1] and guided["truncated"] == 0
        for q in range(3):
            if q == PC.S3_NONE:
                assert guided["expanded"][q] == plain["expanded"][q]
            else:
                assert 2 * guided["expanded"][q] < plain["expanded"][q]
    cells, U1, U2, start, goal, acts2, pri2 = PC.s2_case()
    assert pri2["n_steps"] == 16 and np.all(np.isfinite(pri2["togo"])) and pri2["T"] == 4.0
