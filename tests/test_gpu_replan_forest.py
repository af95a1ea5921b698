"""GPU: the decision passes of the rebase (replan_init_kernel, replan_resolve_kernel, replan_apply_kernel, the scan,
replan_emit_kernel) on the hand-built forests of tests/replan_forest_cases.py -- chains of up to 8192 edges in either id
direction and along a permutation, cycles with tails, a forest of three queries over four tiles, a table whose host-side
bound exceeds its node count, a predecessor that is no node -- against tests/replan_model.py, exactly: the result, the
frontier (ids, g, every state row, count), the rewritten node arrays, the rows behind the count, the spare and the rows
of the node arrays past n_nodes.  check_edges = 0 throughout: no map, no oracle.  What the cases are is held on the models
alone in tests/test_replan_forest_cases.py."""
import numpy as np
import pytest

import replan_forest_cases as FC
import replan_model as RM
from table_model import TableModel
from test_gpu_open import PAT_D, PAT_I, assert_spare_untouched, patterned_frontier, rest_env
from test_gpu_replan import assert_rebased_equal, rebase_both, restore
from test_gpu_table import assert_frontier_equal, bits, upload, upload_lists

pytestmark = pytest.mark.gpu

SPARE_NODES = 3   # rows the table owns behind the case's n nodes
POISON = 0xAB


def states_of(n):
    """n distinct states at rest, one metre apart on a grid 128 wide: one node each, in column order."""
    st = np.zeros((10, n))
    st[0], st[1] = np.arange(n) % 128, np.arange(n) // 128
    return st


def seeded(m, env, case):
    """A table of case.n nodes, node i made from column i with the case's query: (table, download)."""
    tab = env.alloc_table(case.n + SPARE_NODES, n_queries=case.Q)
    st = states_of(case.n)
    tmp = m.TableFrontier(env, case.n)
    assert tab.seed(st, 1.0, frontier=tmp, query=case.query if case.Q > 1 else None) == case.n
    tmp.free()
    d = tab.download()
    assert d["n_nodes"] == case.n and d["status"] == 0
    assert np.array_equal(bits(d["state"]), bits(st)) and len(set(d["hash"].tolist())) == case.n  # ids follow column order
    assert np.array_equal(d["query"], case.query) and np.all(d["pred"] == -1) and np.all(d["g"] == 1.0)
    return tab, d


def relaxed_past_the_bound(m, env, case):
    """The table of FC.bound_lists(): a seed, then one relax the host does not wait for, so that the bound it keeps is
    1 + 512 while the table holds 300 nodes.  Nothing that reads the count back may follow before the rebase.  The
    download is the model's (tests/test_gpu_table.py holds the device to it)."""
    start, lists, pid, pg = FC.bound_lists()
    tab = env.alloc_table(1 + FC.BOUND_ROWS * FC.BOUND_S + SPARE_NODES)
    tmp = m.TableFrontier(env, FC.BOUND_ROWS * FC.BOUND_S)
    assert tab.seed(start, frontier=tmp) == 1
    model = TableModel(10)
    model.seed(start, tab.download()["hash"])
    model.relax(lists, pid, pg)
    L, d_pid, d_pg = upload_lists(m, env, lists), upload(env, m, pid), upload(env, m, pg)
    tab.relax(L, d_pid, d_pg, frontier=tmp, want_count=False)
    env.synchronize()
    for b in (L, d_pid, d_pg, tmp):
        b.free()
    d = model.arrays()
    d.update(status=0, query=np.zeros(case.n, np.int32))
    assert d["n_nodes"] == case.n
    return tab, d


def node_rows(tab, first, count):
    """The bytes of rows [first, first + count) of g, pred and pred_action."""
    v = tab.view()
    return [tab._read(ptr + size * first, np.uint8, size * count) for ptr, size in ((v.g, 8), (v.pred, 4), (v.pred_action, 4))]


def poison_rows(m, tab, first, count):
    v = tab.view()
    for ptr, size in ((v.g, 8), (v.pred, 4), (v.pred_action, 4)):
        a = np.full(size * count, POISON, np.uint8)
        m._abi.check(tab._env._ctx, m._abi.lib().mplx_memcpy_h2d(tab._env._ctx, int(ptr + size * first), a.ctypes.data, a.nbytes))


@pytest.mark.parametrize("case", FC.cases(), ids=[c.name for c in FC.cases()])
def test_rebase_of_a_hand_built_forest(engine, case):
    m = engine
    n, Q = case.n, case.Q
    env = rest_env(m)
    tab, base = relaxed_past_the_bound(m, env, case) if case.name == "bound_above_n" else seeded(m, env, case)
    d0 = case.arrays(base)
    behind = tab.capacity - n
    poison_rows(m, tab, n, behind)  # the rows [n_nodes, bound) and the spare rows of the node arrays
    for s in case.settings:
        what = "%s/%s" % (case.name, s.name)
        args = dict(root=s.root) if Q == 1 else dict(roots=s.roots)
        if s.capacity is not None:
            # a frontier that ends inside the third tile: FRONTIER_FULL, the full n_kept, the first `capacity` kept nodes
            restore(m, tab, d0)
            model = RM.table_from_arrays(d0, Q)
            want_fr, want, status = RM.rebase(model, None, 0, check_edges=False, capacity=s.capacity, **s.args())
            assert status == RM.FRONTIER_FULL and want_fr["count"] == s.capacity < want["n_kept"]
            fr = patterned_frontier(m, env, s.capacity, 32)
            got = tab.rebase(check_edges=False, frontier=fr, **args)
            assert got == want, "%s: %r != %r" % (what, got, want)
            assert tab.stats() == (n, m.table.FRONTIER_FULL), what
            assert int(fr.count.download(np.int64, (1,))[0]) == s.capacity, what
            assert_frontier_equal(fr.download(), want_fr, what)
            assert_spare_untouched(fr, what)
            v, w = tab.view(), model.arrays()
            assert np.array_equal(bits(tab._read(v.g, np.float64, n)), bits(w["g"])), what
            assert np.array_equal(tab._read(v.pred, np.int32, n), w["pred"]), what
            assert np.array_equal(tab._read(v.pred_action, np.int32, n), w["pred_action"]), what
            fr.free()
            assert s is case.settings[-1]  # (the table has its status bit now)
            continue
        fr, want_fr, model, want = rebase_both(m, env, tab, d0, None, 0, what, check_edges=False, n_queries=Q, **args)
        for k, v in s.want.items():
            if k != "depth":
                assert want[k] == v, (what, k)
        # the same call on the rewritten table: the same bytes, and what the model says of its own output
        first_rows, first_fr = node_rows(tab, 0, n), fr.download()
        want_fr2, want2, status = RM.rebase(model, None, 0, check_edges=False, **s.args())
        fr2 = patterned_frontier(m, env, n, 32)
        got2 = tab.rebase(check_edges=False, frontier=fr2, **args)
        assert status == 0 and got2 == want2 and got2["n_kept"] == want["n_kept"], "%s again: %r != %r" % (what, got2, want2)
        assert all(np.array_equal(a, b) for a, b in zip(first_rows, node_rows(tab, 0, n))), what + " again"
        assert_frontier_equal(fr2.download(), first_fr, what + " again")
        assert_frontier_equal(fr2.download(), want_fr2, what + " again")
        assert np.all(fr2.id.download(np.int32, (fr2.state_stride,))[want["n_kept"]:] == PAT_I), what + " again"
        assert np.all(fr2.g.download(np.float64, (fr2.state_stride,))[want["n_kept"]:] == PAT_D), what + " again"
        assert_rebased_equal(tab, model, what + " again")
        fr.free()
        fr2.free()
        assert all(np.all(r == POISON) for r in node_rows(tab, n, behind)), what + ": rows past n_nodes"
    assert all(np.all(r == POISON) for r in node_rows(tab, n, behind)), case.name + ": rows past n_nodes"
    tab.free()
    env.close()
