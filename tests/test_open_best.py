"""CPU: the semantics of include/mplx_best.h as tests/open_best_model.py restates them -- the k cut is a sort by (key bits,
id), a k that cuts nothing is the plain select, and on the corridor of the reference's test_planner_2d k = 16 reaches
nearly the rounds of the default delta with nearly the expansions of delta = 0 -- plus the plumbing of the new header.
Successors come from the CPU oracle; no GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import open_best_model as BM
import open_model as OM
from oracle import oracle as O
from table_model import TableModel
from test_open import corridor_setup, hand_model
from test_table import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf

# (eps, delta, k) -> rounds, expanded, nodes, goal_f; no ray trace, capacity 65 536 (never reached)
CORRIDOR_BEST = {
    (1.0, INF, 1): (586, 586, 1780, 356.5),
    (1.0, INF, 16): (41, 633, 1947, 356.5),
    (1.0, INF, 64): (35, 2121, 5448, 356.5),
    (1.0, INF, 256): (35, 8237, 13229, 356.5),
    (1.0, 10.0, 64): (35, 2070, 5325, 356.5),
    (1.0, 10.0, 256): (35, 6073, 10102, 356.5),  # no cut is ever needed: the default search
    (1.0, 0.0, 16): (69, 589, 1794, 356.5),
    (2.0, INF, 64): (35, 2121, 5303, 361.5),
}


def corridor_best(engine, eps, delta, k, capacity=65536, **kw):
    c, table, opn, prov, start, h0 = corridor_setup(engine)
    opn.__class__ = BM.OpenBestModel
    return table, opn, BM.search_best(table, opn, prov, start, h0, eps, delta, k, capacity, **kw)


@pytest.mark.parametrize("case", sorted(CORRIDOR_BEST))
def test_corridor_with_k_best(engine, case):
    eps, delta, k = case
    rounds, expanded, nodes, goal_f = CORRIDOR_BEST[case]
    table, opn, out = corridor_best(engine, eps, delta, k)
    res = out["result"]
    print(case, out["rounds"], out["expanded"], out["nodes"], res)
    assert out["status"] == OM.FOUND and res["goal_g"] == 351.5 and res["goal_f"] == goal_f
    assert (out["rounds"], out["expanded"], out["nodes"]) == (rounds, expanded, nodes)


def test_k_that_cuts_nothing_is_the_plain_select():
    """The calls of the hand-built scenario through OpenModel.select and select_best with k = the node count: results,
    frontiers, f and flags bit for bit."""
    table, model, states, goal, in_goal, ignored, push1, push2 = hand_model(O)
    table2, best, *_ = hand_model(O)
    best.__class__ = BM.OpenBestModel

    def both(delta, cap, what):
        (want, wfr), (got, gfr) = model.select(delta, cap), best.select_best(OM.HAND_N, delta, cap)
        assert got == want, what
        assert np.array_equal(gfr["id"], wfr["id"]) and gfr["g"].tobytes() == wfr["g"].tobytes(), what
        assert gfr["state"].tobytes() == wfr["state"].tobytes(), what
        assert best.f == model.f and best.flags == model.flags, what
        return want

    for m in (model, best):
        m.push(OM.hand_frontier(states, push1, with_tail=True), len(push1["id"]), 1.0)
    for delta, cap in OM.HAND_SELECTS:
        both(delta, cap, "select(%r, %d)" % (delta, cap))
    for m in (model, best):
        m.push(OM.hand_frontier(states, push2, with_tail=True), 10 ** 9, 1.0, capacity=len(push2["id"]))
    for n in range(200):
        if both(2.5, 5000, "select %d after push 2" % n)["status"] != OM.SELECTED:
            break
    assert n > 5


def test_the_k_cut_takes_the_smallest_keys_and_then_the_smallest_ids():
    states = BM.rest_states(12)
    table = TableModel(10)
    table.seed(states, [O.lattice_hash(2, O.ACC, states[:, i]) for i in range(12)])
    far = np.zeros(10)
    far[:2] = 1000.0
    opn = BM.OpenBestModel(table, 2, far, O.lattice_hash(2, O.ACC, far), 10.0, 1.0)
    keys = [3.0, 1.0, 2.0, 2.0, 5.0, 2.0, 1.0, 2.0, 9.0, 2.0, 0.0, 2.0]
    opn.push(BM.planted(states, keys), 12, 0.0)
    res, fr = opn.select_best(5, INF, 12)  # 0.0, 1.0 twice, and the two smallest ids of the six nodes at 2.0
    assert fr["id"].tolist() == [1, 2, 3, 6, 10] and (res["count"], res["n_open"], res["f_min"]) == (5, 7, 0.0)
    res, fr = opn.select_best(3, 0.5, 12)  # C = the nodes at 2.0 that are left: ids 5, 7, 9, 11
    assert fr["id"].tolist() == [5, 7, 9] and res["f_min"] == 2.0
    res, fr = opn.select_best(3, 1.0, 2)  # C = {11 (2.0), 0 (3.0)}: no k cut; the capacity cut by id
    assert fr["id"].tolist() == [0, 11] and res["n_open"] == 2
    with pytest.raises(ValueError):
        opn.select_best(0, 0.0, 4)


def test_the_key_patterns_cover_what_they_claim():
    pats = BM.key_patterns()
    assert all(k.shape == (BM.PATTERN_N,) and np.all(k >= 0) and not np.isnan(k).any() for k, _ in pats.values())
    assert np.unique(pats["equal"][0]).size == 1
    b = np.sort(pats["low_bits"][0].view(np.uint64))
    assert np.all(np.diff(b) == 1) and b[-1] - b[0] == BM.PATTERN_N - 1 and b[-1] >> 16 == b[0] >> 16
    e = pats["exponents"][0]
    assert np.unique(e).size == 2049 and e.min() == 0.0 and e.max() == INF and 5e-324 in e and 2.0 ** 1023 in e
    r = pats["random"][0].view(np.uint64)
    assert np.isfinite(pats["random"][0]).all() and np.unique(r >> 56).size > 100
    assert (pats["one_below"][0] == 1.0).sum() == 1 and (pats["one_above"][0] == 2.0).sum() == 1


def test_every_function_of_the_header_is_declared_in_abi(engine):
    syms = _declared("mplx_best.h")
    assert syms == ["mplx_open_select_best_device", "mplx_open_select_best_multi_device"]
    assert sorted(engine._abi.BEST_SYMBOLS) == syms
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None and len(getattr(lib, s).argtypes) == 6, s


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_best.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
