"""No GPU: the hand-built forests of tests/replan_forest_cases.py are what they claim to be.  Conditions, not measurements,
held on the models alone: replan_model.rebase (the reference of tests/test_gpu_replan_forest.py) and the descent from the
roots agree on every case and root setting, the counts and depths are those the shapes imply, the forest mixes ids, depths,
queries and tiles, and the restated doubling needs the passes the header promises -- never more than ceil(log2 n) + 1,
exactly k + 1 for a chain of 2^k edges, and no number of passes for a cycle."""
import math

import numpy as np
import pytest

import replan_forest_cases as FC

CASES = FC.cases()
CALLS = [(c, s) for c in CASES for s in c.settings]
IDS = ["%s-%s" % (c.name, s.name) for c, s in CALLS]


@pytest.mark.parametrize("case,setting", CALLS, ids=IDS)
def test_the_two_references_agree_and_the_shape_is_the_claimed_one(case, setting):
    n = case.n
    table, fr, res, status = FC.reference(case, setting)
    kept = FC.kept_by_descent(case, setting)
    ids = np.nonzero(kept)[0]
    root = FC.is_root(case, setting)
    assert res["n_kept"] == ids.size and res["n_roots"] == int(root.sum())
    assert res["n_bad_edges"] == int((FC.bad_without_check(case) & ~root).sum())
    if setting.capacity is None:
        assert status == 0 and np.array_equal(fr["id"], ids)
    else:
        assert status == FC.RM.FRONTIER_FULL and fr["count"] == setting.capacity < ids.size
        assert np.array_equal(fr["id"], ids[:setting.capacity])
        assert 2 * FC.TILE <= ids[setting.capacity] < 3 * FC.TILE  # the cut falls inside the third tile
    # apply: dropped nodes are reset, kept roots lose their back-pointer, and nothing else changes
    g, pred, act = np.array(table.g), np.array(table.pred), np.array(table.pred_action)
    assert np.all(np.isinf(g[~kept])) and np.all(pred[~kept] == -1) and np.all(act[~kept] == -1)
    assert np.all(pred[root] == -1) and np.all(act[root] == -1)
    rest = kept & ~root
    assert np.array_equal(g[kept], case.g[kept]) and np.array_equal(pred[rest], case.pred[rest]) and np.array_equal(act[rest], case.pred_action[rest])
    assert np.all((case.pred_action[rest] >= 0) & (case.pred_action[rest] < FC.N_ACTIONS))
    depth = FC.depth_of_kept(case, setting)
    for k, v in setting.want.items():
        assert {"depth": depth}.get(k, res.get(k)) == v, (k, v, res, depth)
    share = ids.size / n
    if case.family in ("cycles", "forest"):
        assert 0.2 <= share <= 0.8, share
    if case.family == "chain_headless":
        assert math.isinf(case.g[0]) and case.pred[0] == -1 and np.all(np.isfinite(case.g[1:]))
    else:
        assert np.all(np.isfinite(case.g)) or case.family == "forest"
    print("%s: n %d kept %d (share %.3f) roots %d deepest kept chain %d" % (case.name + "/" + setting.name, n, ids.size, share,
                                                                             res["n_roots"], depth))


@pytest.mark.parametrize("case,setting", CALLS, ids=IDS)
def test_passes_needed(case, setting):
    n = case.n
    P = FC.passes_of_bound(n)
    need, settled, dec = FC.doubling(case, setting)
    print("%s: passes needed %s (the part that is no cycle: %d) of P = %d" % (case.name + "/" + setting.name, need, settled, P))
    assert (need is None) == setting.cycle
    assert settled <= P
    # cut after P passes, with what is still UNKNOWN dropped, the doubling is the descent
    _, _, dec_p = FC.doubling(case, setting, limit=P)
    assert np.array_equal(dec_p == FC.KEEP, FC.kept_by_descent(case, setting))
    if need is not None:
        assert need <= P and np.array_equal(dec == FC.KEEP, FC.kept_by_descent(case, setting))
    if case.family == "chain_up" and setting.name == "seeds" and n >= 2 and (n - 1) & (n - 2) == 0:
        assert need == FC.ceil_log2(n - 1) + 1 == P - 1  # n = 2^k + 1: k + 1 passes, one to spare
    if case.family.startswith("chain") and case.family != "chain_headless" and setting.name == "seeds":
        assert need == FC.ceil_log2(n) and FC.doubling(case, setting, limit=need - 1)[0] is None  # d edges: ceil(log2(d + 1))


def test_the_case_list_is_the_one_the_gpu_test_runs():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert [c.n for c in CASES if c.family == "chain_up"] == [2, 3, 5, 64, 65, 257, 4096, 4097, 8193]
    assert [c.n for c in CASES if c.family == "chain_down"] == [65, 4097, 8193]
    assert [c.n for c in CASES if c.family == "chain_shuffled"] == [4097, 8193] and FC.case("chain_headless-4097").n == 4097
    assert FC.case("forest").n == 3 * 4096 + 5 and FC.case("forest").Q == 3 and FC.case("bound_above_n").n == 300
    assert FC.case("pred_out_of_range").n == 5 and 2 * 4096 + 200 < FC.case("cycles").n < 2 * 4096 + 1000
    c = FC.case("chain_down-4097")
    assert np.all(c.pred[:-1] == np.arange(1, c.n)) and c.pred[-1] == -1  # every predecessor has the larger id
    c = FC.case("chain_shuffled-8193")
    assert 0.4 < (c.pred > np.arange(c.n)).mean() < 0.6


def cycle_members(case, ids):
    """True when following pred from ids[0] goes through exactly `ids` and comes back."""
    seen, cur = [], int(ids[0])
    for _ in range(len(ids)):
        seen.append(cur)
        cur = int(case.pred[cur])
    return cur == int(ids[0]) and sorted(seen) == sorted(int(i) for i in ids)


@pytest.mark.parametrize("name", ["cycles", "forest"])
def test_the_cycles_are_there(name):
    case = FC.case(name)
    assert sorted(case.where) == sorted(FC.CYCLE_LENGTHS)
    on_cycle = np.zeros(case.n, bool)
    for L, ids in case.where.items():
        assert len(ids) == L and cycle_members(case, ids)
        on_cycle[ids] = True
    # tails of 1 and of 70 nodes hang off every cycle: walk up from every node that is on no cycle and has no child
    has_child = np.zeros(case.n, bool)
    has_child[case.pred[case.pred >= 0]] = True
    lengths = {L: set() for L in case.where}
    owner = {int(i): L for L, ids in case.where.items() for i in ids}
    for leaf in np.nonzero(~has_child & ~on_cycle & (case.pred >= 0))[0]:
        k, cur = 0, int(leaf)
        while not on_cycle[cur] and case.pred[cur] >= 0:
            cur, k = int(case.pred[cur]), k + 1
        if on_cycle[cur]:
            lengths[owner[cur]].add(k)
    assert all(v == set(FC.TAILS) for v in lengths.values()), lengths
    big = np.array(case.where[4097])
    assert len(set((big // FC.TILE).tolist())) >= 2  # the long cycle spans tiles
    if name == "cycles":
        # with the seeds as roots every cycle and tail is dropped; a root on the 65-cycle keeps that cycle and its tails
        seeds, on65 = case.settings
        kept = FC.kept_by_descent(case, seeds)
        assert not kept[on_cycle].any() and kept.sum() == FC.CYCLES_SEED_CHAIN
        kept = FC.kept_by_descent(case, on65)
        assert kept[case.where[65]].all() and not kept[[i for L in (2, 3, 64, 4097) for i in case.where[L]]].any()
        assert kept.sum() == 65 + FC.CYCLES_TAIL_PAIRS_65 * sum(FC.TAILS)
        table, _, _, _ = FC.reference(case, on65)
        assert table.pred[on65.root] == -1 and table.g[on65.root] == case.g[on65.root]


def test_the_forest_mixes_ids_depths_queries_and_tiles():
    case = FC.case("forest")
    n = case.n
    assert np.array_equal(case.query, np.arange(n) % 3)
    assert 0.3 <= (case.pred > np.arange(n)).mean() <= 0.7
    seeds = case.pred == -1
    print("forest: seeds %.4f, of them with g = +inf %.4f of all nodes; pred > id %.3f" % (
        seeds.mean(), (seeds & np.isinf(case.g)).mean(), (case.pred > np.arange(n)).mean()))
    assert 0.015 <= (seeds & np.isfinite(case.g)).mean() <= 0.025 and 0.007 <= (seeds & np.isinf(case.g)).mean() <= 0.013
    assert np.all(np.isfinite(case.g[~seeds]))
    for s in case.settings:
        kept = FC.kept_by_descent(case, s)
        assert FC.depth_of_kept(case, s) >= 12, s.name
        for t in range(4):
            tile = kept[t * FC.TILE:(t + 1) * FC.TILE]
            assert tile.any() and not tile.all(), (s.name, t)
        waves = [set(case.query[w:w + 64][kept[w:w + 64]].tolist()) for w in range(0, n, 64)]
        if s.name != "seeds-none-foreign":  # (that call keeps query 0 alone)
            assert any(len(w) == 3 for w in waves), s.name
    # the roots of the second call are three edges down; the third call names a seed that was never reached and a kept
    # node of another query
    for q, r in enumerate(case.settings[1].roots):
        assert case.query[r] == q
        assert case.pred[case.pred[case.pred[r]]] >= 0 and case.pred[case.pred[case.pred[case.pred[r]]]] == -1
    _, dead, foreign = case.settings[2].roots
    assert case.query[dead] == 1 and case.pred[dead] == -1 and math.isinf(case.g[dead])
    assert case.query[foreign] == 0 and FC.kept_by_descent(case, case.settings[2])[foreign]
    kq = case.query[FC.kept_by_descent(case, case.settings[2])]
    assert set(kq.tolist()) == {0}


def test_bound_lists_make_the_nodes_the_case_is_written_for():
    from table_model import TableModel
    start, lists, pid, pg = FC.bound_lists()
    t = TableModel(10)
    t.seed(start, [7])
    t.relax(lists, pid, pg)
    assert t.n_nodes == FC.BOUND_N == FC.case("bound_above_n").n
    bound = 1 + FC.BOUND_ROWS * FC.BOUND_S  # what the host can say without waiting for the count
    assert bound > FC.BOUND_N and FC.passes_of_bound(bound) % 2 != FC.passes_of_bound(FC.BOUND_N) % 2
    assert len(set(lists["hash"].tolist())) == FC.BOUND_N - 1 and 7 not in lists["hash"]
