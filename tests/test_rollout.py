"""CPU: the rollout entry points (include/mplx_rollout.h) are declared, exported and bound; the model the GPU tests
compare with (rollout_model.chain) reproduces a result the reference itself holds; and the generated test inputs keep
every terminal class populated."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rollout_model as RM
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_header_symbols_and_binding(engine):
    text = open(os.path.join(ROOT, "include", "mplx_rollout.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["mplx_rollout", "mplx_rollout_device"]
    assert "MPLX_ROLLOUT_BAD_ACTION = 4" in text and "MPLX_ROLLOUT_HEADING_BAND = 0x80" in text
    lib = C.CDLL(engine._abi.LIB_PATH)
    for s in declared:
        assert hasattr(lib, s), "libmplx.so does not export %s" % s
    assert sorted(engine._abi.ROLLOUT_SYMBOLS) == declared
    assert not set(engine._abi.ROLLOUT_SYMBOLS) & set(engine._abi.SYMBOLS)
    L = engine._abi.lib()
    for s in declared:
        assert getattr(L, s).argtypes is not None and len(getattr(L, s).argtypes) == 9
    assert L.mplx_abi_version() == 9
    assert (engine.ROLLOUT_BAD_ACTION, engine.ROLLOUT_HEADING_BAND) == (4, 0x80)
    # mplx_rollout_out: 8 pointers + end_stride
    assert C.sizeof(engine._abi.RolloutOut) == 9 * 8
    assert engine._abi.RolloutOut.end_stride.offset == 5 * 8
    # a NULL context is an argument error, not a crash
    assert L.mplx_rollout(None, None, 1, 1, None, 0, 1, 0, None) == engine._abi.ERR_ARG
    assert L.mplx_rollout_device(None, None, 1, 1, None, 0, 1, 0, None) == engine._abi.ERR_ARG
    # MapPlanner.checkTraj needs the engine's own env
    assert hasattr(engine.MapPlanner, "checkTraj") and hasattr(engine.EnvMap, "rollout") and hasattr(engine.EnvMap, "rollout_resident")


def test_chain_reproduces_the_known_answer_plan(engine):
    """The corridor plan of tests/test_plan_known_answer.py (oracle provider, no device): its start state and its
    actions through chain() give the plan back -- complete, 35 steps, g = 351.5 bit for bit (A* forms g by the same
    adds in the same order, graph_search.h:107), the end state the trajectory's own."""
    from test_plan_known_answer import corridor, run_c1
    ok, s, traj, _ = run_c1(engine)
    assert ok and s["segments"] == 35
    c = corridor()
    U = engine.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    oenv = O.Env(2, O.ACC, U, c["cells"], c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    starts = np.ascontiguousarray(traj.nodes[0], dtype=np.float64).reshape(-1, 1)
    actions = np.ascontiguousarray(traj.actions, dtype=np.int32).reshape(-1, 1)
    for ref in ([False, True] if os.path.exists(O.REF_SO) else [False]):
        r = RM.chain(oenv, starts, actions, ref=ref)
        assert r["status"][0] == 1 and r["steps"][0] == s["segments"] == 35
        assert r["cost"][0] == s["cost"] == 351.5 and r["prefix_cost"][0] == 351.5
        assert np.array_equal(r["end_state"][:, 0].view(np.uint64), np.ascontiguousarray(traj.end).view(np.uint64))
        assert r["end_state"][:, 0].tolist() == [36.5, 3.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 35.0]
        assert int(r["end_hash"][0]) == O.lattice_hash(2, O.ACC, traj.end)
        # every intermediate state is the trajectory's own node
        for k in (1, 17, 34):
            rk = RM.chain(oenv, starts, actions[:k], ref=ref)
            assert rk["steps"][0] == k and np.array_equal(rk["end_state"][:, 0], traj.nodes[k])
    # the model's stops: a wall in the way of segment 20, a bad action, an early end
    cell = np.round((traj.nodes[20][:2] + 0.5 * (traj.nodes[21][:2] - traj.nodes[20][:2]) - np.array(c["origin"])) / c["res"] - 0.5).astype(int)
    cells = c["cells"].copy()
    cells[cell[0] + c["dim"][0] * cell[1]] = 100
    walled = O.Env(2, O.ACC, U, cells, c["dim"], c["origin"], c["res"], v_max=1.0, a_max=1.0, dt=1.0)
    r = RM.chain(walled, starts, actions)
    assert r["status"][0] == 2 and r["steps"][0] == 20 and np.isinf(r["cost"][0]) and np.isfinite(r["prefix_cost"][0])
    bad = actions.copy()
    bad[5] = 9
    r = RM.chain(oenv, starts, bad)
    assert r["status"][0] == 4 and r["steps"][0] == 5
    bad[5] = -1
    r = RM.chain(oenv, starts, bad)
    assert r["status"][0] == 1 and r["steps"][0] == 5 and np.isfinite(r["cost"][0])


@pytest.mark.parametrize("name,scale,tunnel,single", RM.CASES, ids=RM.CASE_IDS)
def test_generated_inputs_populate_every_terminal_class(name, scale, tunnel, single):
    """The caps of the GPU comparison hold on the model alone, for every workload: >= 5 % of the rollouts complete,
    >= 5 % end BLOCKED, >= 5 % end SKIP_DYN (C2-VEL has no limit) -- a change of workloads.py cannot silently empty
    a class on the GPU box."""
    wl, starts, actions, ref = RM.case(name, scale, tunnel, single)
    assert starts.shape == (4 * wl.dim + 2, RM.K) and actions.shape == (RM.H, RM.K) and actions.dtype == np.int32
    assert np.all(starts[wl.dim:] == 0.0)
    if single:
        assert np.all(starts == starts[:, :1])
    lens = (actions >= 0).sum(axis=0)
    assert lens.min() >= 1 and lens.max() == RM.H
    assert np.array_equal((ref["status"] == 1), (ref["steps"] == lens))
    print(name, "shares same/complete/blocked/dyn: %.3f %.3f %.3f %.3f" % RM.shares(ref["status"]), "mean steps %.2f" % ref["steps"].mean())
    RM.check_shares(name, ref["status"])
