"""GPU: the node table and the open set past 1024 scan tiles (more than 4 M entries and nodes), where a thread of the
scans of table_kernel.hip and open_kernel.hip owns two tiles, against the array references of tests/table_model.py and
tests/open_model.py on the scenario of tests/large_case.py (its properties: tests/test_table.py, tests/test_open.py).
Every comparison is bit for bit, as in tests/test_gpu_table.py and tests/test_gpu_open.py; the expected status is 0
throughout.  The lists are uploaded and the reference is computed once for the module, and the fixture asserts the
scenario's conditions on the reference before any test runs.  Every test frees what it allocated, failed or not."""
import math
from contextlib import ExitStack
from types import SimpleNamespace

import numpy as np
import pytest

import large_case as LC
import open_model as OM
from test_gpu_open import (assert_open_equal, assert_result_equal, assert_spare_untouched, patterned_frontier, rest_env,
                           upload_frontier)
from test_gpu_table import assert_frontier_equal, bits, upload, upload_lists

pytestmark = pytest.mark.gpu

ENTRIES = {"A": LC.ROWS_A * LC.S, "B": LC.ROWS_B * LC.S, "C": LC.N_ROWS * LC.S}


def owner(stack):
    """keep(b): b, freed when the stack unwinds (in reverse order: open sets before their tables)."""
    def keep(b):
        stack.callback(b.free)
        return b
    return keep


@pytest.fixture(scope="module")
def big(engine, oracle_lib):
    """The scenario, its reference, and on the device: a context with the goal, the lists of all rows (A is their
    prefix), those of B, and every call's parents."""
    m = engine
    goal_hash = oracle_lib.lattice_hash(2, oracle_lib.ACC, LC.goal_row())
    sc, snaps = LC.reference(goal_hash)
    LC.assert_table_conditions(sc, snaps)
    LC.assert_open_conditions(sc, snaps, goal_hash)
    env = rest_env(m)
    with ExitStack() as stack:
        stack.callback(env.close)
        keep = owner(stack)
        env.set_goal(LC.goal_row(), tol_pos=LC.TOL)
        lists = {"all": keep(upload_lists(m, env, sc["all"])),
                 "B": keep(upload_lists(m, env, LC.rows_of(sc["all"], LC.ROWS_A, LC.ROWS_B)))}
        parents = {name: (keep(upload(env, m, pid.astype(np.int32))), keep(upload(env, m, pg.astype(np.float64))))
                   for name, _, _, pid, pg in sc["calls"]}
        yield SimpleNamespace(m=m, env=env, sc=sc, snaps=snaps, goal_hash=goal_hash, lists=lists, parents=parents)


def relax_call(big, tab, name, frontier, entry_id=None, want_count=True):
    rows = {"A": LC.ROWS_A, "B": LC.ROWS_B, "C": LC.N_ROWS}[name]
    pid, pg = big.parents[name]
    return tab.relax(big.lists["B" if name == "B" else "all"], pid, pg, math.inf, frontier=frontier, n_nodes=rows,
                     entry_id=entry_id, want_count=want_count)


def first_difference(got, want, n_tiles, what):
    """For the message of a failed comparison: the first differing index, its tile and its scan slice."""
    n = min(len(got), len(want))
    d = np.nonzero(np.asarray(got[:n]) != np.asarray(want[:n]))[0]
    if not d.size:
        return "%s: lengths %d != %d" % (what, len(got), len(want))
    i = int(d[0])
    return "%s: first of %d differences at %d (tile %d, scan slice %d of %d tiles): %r != %r" % (
        what, d.size, i, i // LC.TILE, int(LC.scan_slice(i, n_tiles)), n_tiles, got[i], want[i])


def assert_same(got, want, n_tiles, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.float64:
        got, want = bits(got), bits(want)
    if not np.array_equal(got, want):
        pytest.fail(first_difference(got, want, n_tiles, what))


def assert_snapshot_equal(tab, snap, what):
    got = tab.download()
    assert got["status"] == 0 and got["n_nodes"] == snap.n_nodes, (what, got["status"], got["n_nodes"], snap.n_nodes)
    n_tiles = LC.tiles(snap.n_nodes)
    for k in ("hash", "g", "pred", "pred_action"):
        assert_same(got[k], getattr(snap, k), n_tiles, "%s: %s" % (what, k))
    for f in range(LC.F):
        assert_same(got["state"][f], snap.state[f], n_tiles, "%s: state row %d" % (what, f))


def assert_rows_equal(fr, count, want, n_tiles, what):
    """The frontier a call wrote against the reference's rows (ids in order, g, state rows)."""
    got = fr.download(count)
    assert got["count"] == want["count"], (what, got["count"], want["count"])
    assert_same(got["id"], want["id"], n_tiles, what + ": frontier ids / order")
    assert_same(got["g"], want["g"], n_tiles, what + ": frontier g")
    assert_frontier_equal(got, want, what)


def test_relax_past_1024_tiles(big):
    """A (1036 entry tiles, per = 2, creating), B (the node count passes 1024 tiles) and C (1133 entry tiles, no new node,
    ties between slices) into one table: n_nodes, status, all node arrays, entry ids and the whole frontier after every
    call; then find on 10 000 hashes."""
    with ExitStack() as stack:
        relax_past_1024_tiles(big, owner(stack))


def relax_past_1024_tiles(big, keep):
    m, env, snaps = big.m, big.env, big.snaps
    tab = keep(env.alloc_table(LC.NODE_CAPACITY))
    fr = keep(m.TableFrontier(env, ENTRIES["C"]))
    d_eid = keep(m.DeviceArray(env, ENTRIES["C"] * 4))
    for name in "ABC":
        snap, n = snaps[name], ENTRIES[name]
        d_eid.upload(np.full(n, -7, np.int32))
        cnt = relax_call(big, tab, name, fr, entry_id=d_eid)
        assert cnt == snap.frontier_id.size, (name, cnt, snap.frontier_id.size)
        assert_snapshot_equal(tab, snap, name)
        assert_same(d_eid.download(np.int32, (n,)), snap.entry_id, LC.tiles(n), name + ": entry ids")
        assert_rows_equal(fr, cnt, snap.frontier(), LC.tiles(n), name)
    final = snaps["C"]
    rng = np.random.default_rng(33)
    ids = np.concatenate([[0, final.n_nodes - 1], rng.choice(final.n_nodes, 9897, replace=False)])
    strangers = np.concatenate([np.uint64(0xDEAD00000000) + np.arange(50, dtype=np.uint64),
                                np.arange(LC.K + 7, LC.K + 57, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)])
    assert not np.isin(strangers, final.hash).any()
    empty_id = int(np.nonzero(final.hash == LC.EMPTY)[0][0])
    got = tab.find(np.concatenate([final.hash[ids], [LC.EMPTY], strangers]))
    assert got.size == 10000 and np.array_equal(got, np.concatenate([ids, [empty_id], np.full(100, -1)]).astype(np.int32))


def test_select_sized_by_the_bound_across_1024_tiles(big):
    """Relax A with a count, B without one, and with no host read in between push B's frontier and select everything:
    the select's grids come from the host's bound min(capacity, nodes after A + entries of B) while the node count, on
    the device, moves from 970 tiles to 1040."""
    with ExitStack() as stack:
        select_sized_by_the_bound(big, owner(stack))


def select_sized_by_the_bound(big, keep):
    m, env, snap = big.m, big.env, big.snaps["B"]
    nodes_a = big.snaps["A"].n_nodes
    assert LC.tiles(nodes_a) < LC.SCAN < LC.tiles(snap.n_nodes) <= LC.tiles(nodes_a + ENTRIES["B"])  # (the last: the bound's)
    tab = keep(env.alloc_table(LC.NODE_CAPACITY))
    opn = keep(env.alloc_open(tab))
    fr_a, fr_b = keep(m.TableFrontier(env, ENTRIES["A"])), keep(m.TableFrontier(env, ENTRIES["B"]))
    sel = keep(patterned_frontier(m, env, LC.NODE_CAPACITY, 64))
    assert relax_call(big, tab, "A", fr_a) == big.snaps["A"].frontier_id.size
    fr_a.free()
    assert relax_call(big, tab, "B", fr_b, want_count=False) is None
    opn.push(fr_b, n_max=ENTRIES["B"], eps=1.0)
    got = opn.select(math.inf, sel)
    model = LC.open_reference(snap, big.goal_hash)
    model.push(snap.frontier(), ENTRIES["B"], 1.0)
    want, want_sel = model.select(math.inf, LC.NODE_CAPACITY)
    assert_result_equal(got, want, "select")
    assert tab.stats() == (snap.n_nodes, 0)
    assert_rows_equal(sel, None, want_sel, LC.tiles(snap.n_nodes), "select")
    assert_rows_equal(fr_b, None, snap.frontier(), LC.tiles(ENTRIES["B"]), "B")
    assert_spare_untouched(sel)
    assert_open_equal(opn, model, "after the select")


def test_push_and_select_over_1040_node_tiles(big):
    """The frontier of C pushed into the open set of the full table, the selects of large_case.SELECTS into patterned
    frontiers, then the second push and FOUND by the smallest of the tied goal nodes."""
    with ExitStack() as stack:
        push_and_select(big, owner(stack))


def push_and_select(big, keep):
    m, env, sc, snap = big.m, big.env, big.sc, big.snaps["C"]
    n_tiles = LC.tiles(snap.n_nodes)
    assert n_tiles > LC.SCAN + 1
    tab = keep(env.alloc_table(LC.NODE_CAPACITY))
    opn = keep(env.alloc_open(tab))
    imp = keep(m.TableFrontier(env, ENTRIES["C"]))
    for name in "AB":
        relax_call(big, tab, name, imp, want_count=False)
    assert relax_call(big, tab, "C", imp) == snap.frontier_id.size and tab.stats() == (snap.n_nodes, 0)
    model = LC.open_reference(snap, big.goal_hash)
    opn.push(imp, n_max=ENTRIES["C"], eps=1.0)
    model.push(snap.frontier(), ENTRIES["C"], 1.0)
    assert_open_equal(opn, model, "push 1")
    d_res = keep(m.DeviceArray(env, 48))
    frs = {cap: keep(patterned_frontier(m, env, cap, 64)) for cap in sorted(set(cap for _, cap in LC.SELECTS))}
    for delta, cap in LC.SELECTS:
        what = "select(%r, %d)" % (delta, cap)
        got = opn.select(delta, frs[cap], d_result=d_res)
        want, want_fr = model.select(delta, cap)
        assert_result_equal(got, want, what)
        assert got["status"] == OM.SELECTED
        assert_rows_equal(frs[cap], None, want_fr, n_tiles, what)
        assert_spare_untouched(frs[cap], what)
        assert_open_equal(opn, model, what)
        r = m._abi.OpenResult.from_buffer_copy(d_res.download(np.uint8, (48,)).tobytes())
        assert (r.status, r.goal_id, r.count, r.n_open) == (got["status"], got["goal_id"], got["count"], got["n_open"])
        assert bits([r.f_min, r.goal_f, r.goal_g]).tolist() == bits([got["f_min"], got["goal_f"], got["goal_g"]]).tolist()
        if (delta, cap) in ((2.5, 16), (80.0, 5000)):  # truncated: a qualifying node with a larger id is still open
            f, fl = model.arrays()
            left = np.nonzero(((fl & OM.IS_OPEN) > 0) & (f <= got["f_min"] + delta))[0]
            assert got["count"] == cap and got["n_open"] > 0 and left.size > 0 and left.max() > want_fr["id"][-1]
    assert got["n_open"] == 0 and got["count"] > 500000
    # the second push: the goal's box at g = 50 among dearer nodes; FOUND by the smallest of the tied ids
    host = LC.push_two(sc, snap)
    fr2 = keep(upload_frontier(m, env, host, host["count"]))
    opn.push(fr2, n_max=host["count"], eps=1.0)
    model.push(host, host["count"], 1.0)
    assert_open_equal(opn, model, "push 2")
    got = opn.select(2.5, frs[5000], d_result=d_res)
    want, want_fr = model.select(2.5, 5000)
    assert_result_equal(got, want, "FOUND")
    f, fl = model.arrays()
    tied = np.nonzero(((fl & OM.IS_GOAL) > 0) & (f == want["goal_f"]))[0]
    assert got["status"] == OM.FOUND and got["count"] == 0 and tied.size >= 2 and got["goal_id"] == tied.min()
    assert np.unique(LC.scan_slice(tied, n_tiles)).size >= 2
    assert_rows_equal(frs[5000], None, want_fr, n_tiles, "FOUND")
    assert_spare_untouched(frs[5000], "FOUND")
    assert_open_equal(opn, model, "FOUND")
