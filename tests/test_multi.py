"""CPU: the semantics of include/mplx_multi.h as tests/multi_model.py restates them.  The property that carries the
feature is separation: query q of a batch, its nodes renumbered by rank, is bit for bit what the single-query models
give for that start and goal -- table rows, open set, the result of every round in which q selected -- as long as no
selection is cut at the frontier's capacity; and a cut batch still ends every query FOUND at the single search's cost.
Plus the plumbing of the new header (declared in _abi.py, exported, parses as C).  Successors come from the CPU oracle;
no GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import multi_model as MM
import open_model as OM
from oracle import oracle as O
from table_model import TableModel, oracle_provider
from test_open import corridor_setup
from test_plan_known_answer import corridor
from test_table import _declared

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def corridor_queries(engine):
    """Three queries on the corridor of test_planner_2d: its own start and goal; both shifted by 0.5 m along free
    cells; and the way back (q2's start is q0's goal and the other way round).  Returns (starts [10][3], goals [3][10])."""
    c = corridor()
    wp = lambda p: engine.Waypoint(2, engine.ACC, pos=p).to_row()
    s0, g0 = np.asarray(c["start"], dtype=np.float64), np.asarray(c["goal"], dtype=np.float64)
    starts = np.stack([wp(s0), wp(s0 + [0.0, 0.5]), wp(g0)], axis=1)
    goals = np.stack([wp(g0), wp(g0 + [0.0, -0.5]), wp(s0)])
    return starts, goals


def assert_same_table(got, want, what=""):
    assert got["n_nodes"] == want["n_nodes"], what
    for k in ("hash", "pred", "pred_action"):
        assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)
    assert np.array_equal(_bits(got["g"]), _bits(want["g"])), what + ": g"
    assert np.array_equal(_bits(got["state"]), _bits(want["state"])), what + ": state"


def assert_same_result(got, want, what=""):
    for k in ("status", "goal_id", "count", "n_open"):
        assert got[k] == want[k], "%s: %s %r != %r" % (what, k, got[k], want[k])
    for k in ("f_min", "goal_f", "goal_g"):
        assert _bits([got[k]])[0] == _bits([want[k]])[0], "%s: %s %r != %r" % (what, k, got[k], want[k])


def single_corridor(engine, start, goal, eps, delta, cap, **kw):
    """OM.search for one start / goal on the corridor, with the result of every round."""
    _, _, _, prov, _, _ = corridor_setup(engine)
    table = TableModel(10)
    opn = OM.OpenModel(table, 2, goal, O.lattice_hash(2, O.ACC, goal), w=10.0, v_max=1.0, tol_pos=0.5)
    history = []
    real_select = opn.select

    def select(delta_, cap_):
        res, fr = real_select(delta_, cap_)
        history.append(dict(res))
        return res, fr
    opn.select = select
    out = OM.search(table, opn, prov, start, O.lattice_hash(2, O.ACC, start), eps, delta, cap, **kw)
    return table, opn, out, history[:out["rounds"]]  # (the selects that led to a relax)


def batch_corridor(engine, starts, goals, eps, delta, cap, **kw):
    _, _, _, prov, _, _ = corridor_setup(engine)
    Q = starts.shape[1]
    table = MM.MultiTableModel(10, Q)
    opn = MM.MultiOpenModel(table, 2, goals, [O.lattice_hash(2, O.ACC, g) for g in goals], w=10.0, v_max=1.0, tol_pos=0.5)
    out = MM.search_many(table, opn, prov, starts, [O.lattice_hash(2, O.ACC, starts[:, q]) for q in range(Q)], eps, delta, cap, **kw)
    return table, opn, out


_singles = {}


def singles(engine, eps, delta):
    """The three single searches, computed once per (eps, delta) and left unchanged."""
    if (eps, delta) not in _singles:
        starts, goals = corridor_queries(engine)
        _singles[(eps, delta)] = [single_corridor(engine, starts[:, q], goals[q], eps, delta, 1 << 16) for q in range(3)]
    return _singles[(eps, delta)]


@pytest.mark.parametrize("delta", [0.0, 2.0])
def test_batch_model_is_three_single_models_under_the_renumbering(engine, delta):
    starts, goals = corridor_queries(engine)
    table, opn, out = batch_corridor(engine, starts, goals, 1.0, delta, 1 << 16)
    assert out["truncated"] == 0 and out["status"] == [MM.FOUND] * 3
    arr = table.arrays()
    f, fl = opn.arrays()
    assert out["results"][0]["goal_g"] == 351.5  # reference README.md:199-202
    for q, (t1, o1, out1, hist1) in enumerate(singles(engine, 1.0, delta)):
        what = "query %d" % q
        sub, fq, flq, rank = MM.restrict(arr, q, f, fl)
        assert_same_table(sub, t1.arrays(), what)
        f1, fl1 = o1.arrays()
        assert np.array_equal(flq, fl1), what
        seen = (fl1 & OM.SEEN) > 0
        assert np.array_equal(_bits(fq[seen]), _bits(f1[seen])), what
        assert out1["status"] == MM.FOUND and (out["rounds"][q], out["expanded"][q]) == (out1["rounds"], out1["expanded"]), what
        assert len(out["history"][q]) == len(hist1)
        for k, (got, want) in enumerate(zip(out["history"][q], hist1)):
            assert_same_result(MM.renumber_result(got, rank), want, "%s round %d" % (what, k))
        assert_same_result(MM.renumber_result(out["results"][q], rank), out1["result"], what + " last")
    assert out["total_rounds"] == max(out["rounds"])
    # the node sets are disjoint and cover the table
    assert sorted(np.concatenate([np.nonzero(arr["query"] == q)[0] for q in range(3)]).tolist()) == list(range(table.n_nodes))


def test_a_cut_batch_still_finds_every_single_cost(engine):
    """Frontier capacity 8: selections are cut in global id order, queries wait for each other, nothing is lost."""
    starts, goals = corridor_queries(engine)
    table, opn, out = batch_corridor(engine, starts, goals, 1.0, 2.0, 8)
    assert out["truncated"] > 10 and out["status"] == [MM.FOUND] * 3
    for q, (_, _, out1, _) in enumerate(singles(engine, 1.0, 2.0)):
        assert out["results"][q]["goal_g"] == out1["result"]["goal_g"], q
    assert out["results"][0]["goal_g"] == 351.5


def hand_models():
    """The hand-built scenario through the batch model: seeds, two crafted relax calls, the pushes and selects between
    them.  Returns what tests/test_gpu_multi.py replays on the device: (table, open set, steps)."""
    states, query, g, goals = MM.hand_seeds()
    hashes = [O.lattice_hash(2, O.ACC, states[:, k]) for k in range(states.shape[1])]
    table = MM.MultiTableModel(10, MM.HAND_Q)
    opn = MM.MultiOpenModel(table, 2, goals, [O.lattice_hash(2, O.ACC, r) for r in goals], MM.HAND_W, MM.HAND_VMAX, tol_pos=MM.HAND_TOL)
    return table, opn, states, query, g, goals, hashes


def test_the_hand_built_scenario_separates_and_covers_what_it_claims():
    table, opn, states, query, g, goals, hashes = hand_models()
    singles_t = [TableModel(10) for _ in range(MM.HAND_Q)]
    singles_o = [OM.OpenModel(t, 2, goals[q], O.lattice_hash(2, O.ACC, goals[q]), MM.HAND_W, MM.HAND_VMAX, tol_pos=MM.HAND_TOL)
                 for q, t in enumerate(singles_t)]

    def check(what):
        arr = table.arrays()
        f, fl = opn.arrays()
        for q in range(MM.HAND_Q):
            sub, fq, flq, _ = MM.restrict(arr, q, f, fl)
            assert_same_table(sub, singles_t[q].arrays(), "%s: query %d" % (what, q))
            f1, fl1 = singles_o[q].arrays()
            assert np.array_equal(flq, fl1) and np.array_equal(_bits(fq[(fl1 & OM.SEEN) > 0]), _bits(f1[(fl1 & OM.SEEN) > 0])), what

    def push_all(fr, per_q):
        opn.push(fr, fr["count"], 1.0)
        for q in range(MM.HAND_Q):
            singles_o[q].push(per_q[q], per_q[q]["count"], 1.0)

    def select_all(delta, what):
        res, sel = opn.select_many(delta, 10 ** 6)
        rank = MM.restrict(table.arrays(), 0)[3]
        for q in range(MM.HAND_Q):
            rank = MM.restrict(table.arrays(), q)[3]
            want, want_sel = singles_o[q].select(delta, 10 ** 6)
            assert_same_result(MM.renumber_result(res[q], rank), want, "%s: query %d" % (what, q))
            mine = sel["id"][np.asarray(table.query)[sel["id"]] == q]
            assert np.array_equal(rank[mine], want_sel["id"]), what
        return res

    fr = table.seed(states, hashes, g, query)[0]
    per_q = [singles_t[q].seed(states[:, query == q], [h for h, qq in zip(hashes, query) if qq == q], g[query == q])[0]
             for q in range(MM.HAND_Q)]
    assert table.n_nodes == 42 and fr["count"] == 42  # 30 + 12 (query, hash) pairs; the three repeats create nothing
    # the same hash in two queries is two nodes
    both = [h for h in set(hashes) if sum(1 for k in table.ids if k[1] == h) == 2]
    assert len(both) == 12
    check("seeds")
    push_all(fr, per_q)
    check("push of the seeds")
    statuses = {r["status"] for r in select_all(0.0, "select 0")}
    rng = np.random.default_rng(17)
    for call in range(2):
        n_before = table.n_nodes
        lists, pid, pg, pool = MM.hand_relax(rng, n_before)
        inside = (pid >= 0) & (pid < n_before)
        row_query = np.where(inside, np.asarray(table.query)[np.where(inside, pid, 0)], -1)
        ranks = [MM.restrict(table.arrays(), q)[3] for q in range(MM.HAND_Q)]
        fr, entry_id = table.relax(lists, pid, pg)
        S = lists["stride"]
        for k in np.nonzero(~inside)[0]:  # a row whose parent is no node of the table touches nothing
            assert np.all(entry_id[k * S:(k + 1) * S] == -1)
        per_q = []
        for q in range(MM.HAND_Q):
            sub, spid, spg = MM.split_rows(lists, pid, pg, row_query, ranks[q], q)
            per_q.append(singles_t[q].relax(sub, spid, spg)[0])
        assert sum(p["count"] for p in per_q) == fr["count"] > 20
        check("relax %d" % call)
        # the hash equal to the empty marker: a node in more than one query
        from table_model import EMPTY
        assert sum(1 for k in table.ids if k[1] == int(EMPTY)) >= 2
        push_all(fr, per_q)
        check("push %d" % call)
        for delta in (0.5, math.inf):
            statuses |= {r["status"] for r in select_all(delta, "select %d %r" % (call, delta))}
    assert {MM.SELECTED, MM.FOUND} <= statuses  # a FOUND query sits still while the others select
    for k in range(50):
        res = select_all(math.inf, "drain %d" % k)
        if not any(r["status"] == MM.SELECTED for r in res):
            break
    assert [r["status"] for r in res] == [MM.FOUND] * 3
    # find: hits per query, misses for a hash another query holds
    keys = list(table.ids)
    hits = table.find([h for _, h in keys], [q for q, _ in keys])
    assert np.array_equal(hits, np.array([table.ids[k] for k in keys], dtype=np.int32))
    only0 = [h for q, h in keys if q == 0 and (1, h) not in table.ids]
    assert only0 and np.all(table.find(only0, [1] * len(only0)) == -1)


def test_every_function_of_the_header_is_declared_in_abi(engine):
    """Fails without the feature: the header, the symbols and the bindings are all new."""
    syms = _declared("mplx_multi.h")
    assert len(syms) == 7 and "mplx_table_create_multi" in syms and "mplx_open_select_multi_device" in syms
    assert sorted(engine._abi.MULTI_SYMBOLS) == syms
    assert not set(syms) & set(engine._abi.TABLE_SYMBOLS + engine._abi.OPEN_SYMBOLS + engine._abi.SYMBOLS)
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s  # exported by the library and bound
    # the structs the new calls take are those of mplx_table.h / mplx_open.h / mplx.h: their layouts as the header states
    assert C.sizeof(engine._abi.OpenResult) == 48 and C.sizeof(engine._abi.TableFrontier) == 6 * 8
    assert C.sizeof(engine._abi.GoalSpec) == 8 + 2 * 4 + 6 * 8
    assert engine._abi.OpenResult.count.offset == 8 and engine._abi.OpenResult.f_min.offset == 24
    assert lib.mplx_open_set_goals.argtypes[1]._type_ is engine._abi.GoalSpec
    assert lib.mplx_open_select_multi_device.argtypes[4]._type_ is engine._abi.OpenResult
    assert hasattr(engine.EnvMap, "search_many") and hasattr(engine.OpenSet, "select_many") and hasattr(engine.OpenSet, "set_goals")
    assert engine.MultiSearchResult is engine.search.MultiSearchResult


def test_header_parses_as_c():
    r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "include", "mplx_multi.h")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
