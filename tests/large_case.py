"""The large scenario of tests/test_gpu_table_large.py: three relax calls that take the node table and the open set past
1024 scan tiles (kTableTile = 4096 entries or nodes per tile, one 1024-thread workgroup scanning the tile counts, so
that a scan thread owns per = ceil(n_tiles / 1024) = 2 tiles), and their array references (tests/table_model.py::
TableArrays, tests/open_model.py::OpenArrays).  A seeded builder, no files.  What the scenario has to contain for the
GPU tests to mean anything is asserted on the references alone, without a GPU, by tests/test_table.py and
tests/test_open.py (assert_table_conditions, assert_open_conditions), and again by the GPU tests' fixture.

Lists: N_ROWS rows x 40 entries over a bare 2D state (10 rows).  Key index i is (i + 1) * 0x9E3779B97F4A7C15 mod 2^64
and sits at (i % W, i // W) on a 0.1 m lattice; the position rows of every entry with that key hold the position, the
other rows hold small exact values of the entry index, so a node that took the state of any entry but its first shows.
Most keys appear once, at a random entry; the other entries repeat keys drawn at random, so copies of a key lie in
tiles that different scan threads own.  Costs from {0.25, 0.5, 1, 1.5, 2} with 0.5 % +inf and 0.5 % NaN, parent_g from
{0, 0.5, 1}, 1 % of the rows with count 0 (their entries look valid), a few rows with a partial count and NaN costs,
NaN states and hashes that exist nowhere else behind it, a parent without id in A and in B, and the hash the table's
key field cannot hold (EMPTY) in four entries of different tiles.

Calls, into one table:
  A  rows [0, ROWS_A): 1036 entry tiles, the last one partial -- per = 2 in a call that creates and improves nodes; it
     leaves fewer than 1024 tiles of nodes
  B  the other rows: new keys and keys of A with equal, larger and smaller candidates; the table passes 1025 node tiles
  C  all rows at once under other parent ids, parent_g lowered by 0.5 for a random third of the parents: every key is
     there, no node is created, and the winners of ties lie in other scan slices than the losers
The halves are unequal because two calls of 530 tiles never reach per = 2 while they still create nodes: only the scan
of the winners would then see two tiles per thread, never the scan that numbers the new nodes.

The open set: the goal is the lattice position of key GOAL_INDEX (chosen once, by looking at the reference, as a place
where all 121 keys of the tolerance box became nodes and enough of the ring around it improved in C; the key of that
index is the goal's lattice hash, so that its node has h = 0).  Entries with a key inside the box cost 100 more, as the
first push of open_model.hand_scenario keeps its goal region dear: the selects before push_two() are SELECTED.
"""
import functools
import math

import numpy as np

import open_model as OM
from table_model import EMPTY, TableArrays

TILE, SCAN = 4096, 1024                # kTableTile; threads of the scan's workgroup
S, F = 40, 10
ROWS_A, ROWS_B = 106000, 10000
N_ROWS = ROWS_A + ROWS_B
KEYS_A, KEYS_B = 4050000, 290000       # keys that appear first in A / in B
K = KEYS_A + KEYS_B
W = 2048                               # lattice width
GOAL_INDEX = 143471
W_HEUR, V_MAX, TOL = 10.0, 1.0, 0.5
NODE_CAPACITY = 4400000
EMPTY_ENTRIES = (5, 3 * TILE + 17, ROWS_A * S - 3, ROWS_A * S + 5000)
# (delta, capacity): those of open_model.HAND_SELECTS; (80, 5000) is a truncated selection with rows in hundreds of slices
SELECTS = [(0.0, 0), (0.0, 16), (2.5, 16), (2.5, 5000), (80.0, 5000), (math.inf, 16), (math.inf, NODE_CAPACITY)]


def tiles(n):
    return (n + TILE - 1) // TILE


def scan_slice(index, n_tiles):
    """The scan thread that owns the tile of entry / node `index` in a scan over n_tiles tiles."""
    return np.asarray(index) // TILE // ((n_tiles + SCAN - 1) // SCAN)


def lattice(key_index):
    key_index = np.asarray(key_index)
    return np.stack([(key_index % W) * 0.1, (key_index // W) * 0.1])


def goal_row():
    g = np.zeros(F)
    g[:2] = lattice(GOAL_INDEX)
    return g


def scenario(goal_hash, seed=31):
    """{"all": lists of all rows, "key_index" per entry, "keys", "in_box" per key index, "calls": per call (name, first
    row, rows, parent_id, parent_g)}.  goal_hash: the lattice hash of goal_row() (2D ACC at rest)."""
    rng = np.random.default_rng(seed)
    N, NA = N_ROWS * S, ROWS_A * S
    keys = np.arange(1, K + 2, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    keys[K] = EMPTY
    keys[GOAL_INDEX] = np.uint64(goal_hash)
    assert np.unique(keys).size == K + 1
    ki = np.empty(N, np.int64)
    ki[:NA] = rng.integers(0, KEYS_A, size=NA)
    ki[rng.choice(NA, KEYS_A, replace=False)] = rng.permutation(KEYS_A)
    ki[NA:] = rng.integers(0, K, size=N - NA)
    ki[NA + rng.choice(N - NA, KEYS_B, replace=False)] = KEYS_A + rng.permutation(KEYS_B)
    ki[list(EMPTY_ENTRIES)] = K
    cost = rng.choice([0.25, 0.5, 1.0, 1.5, 2.0], size=N)
    r = rng.random(N)
    cost[r < 0.005] = np.inf
    cost[(r >= 0.005) & (r < 0.01)] = np.nan
    count = np.full(N_ROWS, S, np.int32)
    count[rng.random(N_ROWS) < 0.01] = 0
    partial = np.concatenate([[1, 2, ROWS_A - 1, ROWS_A, N_ROWS - 1], rng.choice(N_ROWS, 15, replace=False)])
    count[partial] = rng.integers(1, S, size=partial.size)
    count[1] = 1
    parent_g = rng.choice([0.0, 0.5, 1.0], size=N_ROWS)
    lowered = rng.random(N_ROWS) < 1.0 / 3.0
    action = rng.integers(0, 25, size=N).astype(np.int32)
    in_box = np.abs(lattice(np.arange(K + 1)) - goal_row()[:2, None]).max(axis=0) <= TOL
    cost[in_box[ki]] += 100.0
    e = np.arange(N)
    state = np.empty((F, N))
    state[:2] = lattice(ki)
    for f in range(2, F):
        state[f] = ((e + 17 * f) % 509) * 0.125
    hsh = keys[ki]
    dead = np.zeros(N, bool)
    for k in partial:
        dead[k * S + count[k]:(k + 1) * S] = True
    cost[dead] = np.nan
    state[:, dead] = np.nan
    hsh[dead] = np.uint64(0xDEAD00000000) + e[dead].astype(np.uint64)
    assert not np.isin(hsh[dead], keys).any()
    pid = np.arange(N_ROWS, dtype=np.int32)
    pid[[7, ROWS_A + 7]] = -1
    pid_c = np.where(pid < 0, -1, pid + N_ROWS).astype(np.int32)
    pg_c = np.where(lowered, np.maximum(parent_g - 0.5, 0.0), parent_g)
    calls = [("A", 0, ROWS_A, pid[:ROWS_A], parent_g[:ROWS_A]), ("B", ROWS_A, ROWS_B, pid[ROWS_A:], parent_g[ROWS_A:]),
             ("C", 0, N_ROWS, pid_c, pg_c)]
    lists = {"stride": S, "count": count, "action": action, "cost": cost, "hash": hsh, "state": state}
    return {"all": lists, "key_index": ki, "keys": keys, "in_box": in_box, "partial": partial, "calls": calls}


def rows_of(lists, first, rows):
    """The lists of rows [first, first + rows) (views)."""
    a, b = first * S, (first + rows) * S
    return {"stride": S, "count": lists["count"][first:first + rows], "action": lists["action"][a:b],
            "cost": lists["cost"][a:b], "hash": lists["hash"][a:b], "state": lists["state"][:, a:b]}


class Snapshot:
    """The node arrays after a call, as OpenArrays and the comparisons want them.  hash and state are views of the final
    table's (ids and states never change), g / pred / pred_action are the call's own."""

    def __init__(self, table, entry_id, frontier):
        self.n_fields, self.n_nodes = table.n_fields, table.n_nodes
        self._table = table
        self.g, self.pred, self.pred_action = table.g.copy(), table.pred.copy(), table.pred_action.copy()
        self.entry_id = entry_id
        self.frontier_id, self.frontier_g = frontier["id"], frontier["g"]

    @property
    def hash(self):
        return self._table.hash[:self.n_nodes]

    @property
    def state(self):
        return self._table.state[:, :self.n_nodes]

    def frontier(self):
        return {"count": self.frontier_id.size, "id": self.frontier_id, "g": self.frontier_g,
                "state": self.state[:, self.frontier_id]}


@functools.lru_cache(maxsize=1)
def reference(goal_hash):
    """(scenario, {call name: Snapshot}): computed once per process and shared; nobody writes into it."""
    sc = scenario(goal_hash)
    table, snaps = TableArrays(F), {}
    for name, first, rows, pid, pg in sc["calls"]:
        fr, eid = table.relax(rows_of(sc["all"], first, rows), pid, pg)
        snaps[name] = Snapshot(table, eid, fr)
    return sc, snaps


def open_reference(snap, goal_hash):
    return OM.OpenArrays(snap, 2, goal_row(), goal_hash, W_HEUR, V_MAX, tol_pos=TOL)


def push_two(sc, snap, seed=32):
    """The second push: every node of the goal's box but its own cell with g = 50 (nodes at the same distance tie, the
    smallest id wins) among 200 000 other nodes with g from 60 on, in shuffled order."""
    rng = np.random.default_rng(seed)
    box = np.nonzero(sc["in_box"][key_index_of_nodes(sc, snap)])[0]
    box = box[snap.hash[box] != sc["keys"][GOAL_INDEX]]
    rest = np.setdiff1d(rng.choice(snap.n_nodes, 200000, replace=False), box)
    ids = np.concatenate([box, rest])
    g = np.concatenate([np.full(box.size, 50.0), 60.0 + rng.choice(np.arange(8) * 0.5, rest.size)])
    o = rng.permutation(ids.size)
    ids, g = ids[o], g[o]
    return {"count": ids.size, "id": ids.astype(np.int32), "g": g, "state": snap.state[:, ids]}


def key_index_of_nodes(sc, snap):
    """Per node: the index of its key (from the lattice position its state carries)."""
    at = np.rint(snap.state[:2] / 0.1).astype(np.int64)
    ki = at[0] + W * at[1]
    assert np.array_equal(sc["keys"][ki], snap.hash)
    return ki


def best_entries(sc, snaps, name):
    """Of call `name`: (entries whose candidate is the new g of a node the call improved, their node ids)."""
    names = [c[0] for c in sc["calls"]]
    _, first, rows, pid, pg = sc["calls"][names.index(name)]
    snap = snaps[name]
    before = np.full(snap.n_nodes, np.inf)
    if name != "A":
        prev = snaps[names[names.index(name) - 1]]
        before[:prev.n_nodes] = prev.g
    e = np.nonzero(snap.entry_id >= 0)[0]
    ids = snap.entry_id[e]
    cand = np.repeat(pg, S)[e] + rows_of(sc["all"], first, rows)["cost"][e]
    best = (cand == snap.g[ids]) & (snap.g[ids] < before[ids])
    return e[best], ids[best]


def nodes_tied_across_slices(sc, snaps, name):
    """Number of nodes the call improved whose best candidate is shared by entries of different scan slices."""
    e, ids = best_entries(sc, snaps, name)
    sl = scan_slice(e, tiles(snaps[name].entry_id.size))
    lo, hi = np.full(snaps[name].n_nodes, 1 << 40), np.full(snaps[name].n_nodes, -1)
    np.minimum.at(lo, ids, sl)
    np.maximum.at(hi, ids, sl)
    return int((hi > lo).sum())


def assert_table_conditions(sc, snaps):
    """What the relax calls must contain, on the reference alone."""
    A, B, Cc = snaps["A"], snaps["B"], snaps["C"]
    lists = sc["all"]
    # A: more than 1024 entry tiles, the last one partial, in a call that creates and improves nodes; ties between slices
    assert tiles(A.entry_id.size) > SCAN and A.entry_id.size % TILE != 0
    assert A.n_nodes > 0 and A.frontier_id.size == A.n_nodes
    assert nodes_tied_across_slices(sc, snaps, "A") >= 1000
    # the node count crosses 1024 tiles in B, and ends in a partial tile
    assert A.n_nodes < SCAN * TILE and B.n_nodes >= (SCAN + 1) * TILE + 1 and B.n_nodes % TILE != 0
    assert tiles(B.n_nodes) >= SCAN + 2
    # B meets at least 1000 keys of A, with equal, larger and smaller candidates, and creates nodes
    e = np.nonzero(B.entry_id >= 0)[0]
    ids = B.entry_id[e]
    cand = np.repeat(sc["calls"][1][4], S)[e] + rows_of(lists, ROWS_A, ROWS_B)["cost"][e]
    old = ids < A.n_nodes
    assert np.unique(ids[old]).size >= 1000
    for cmp_ in (np.equal, np.greater, np.less):
        assert cmp_(cand[old], A.g[ids[old]]).sum() >= 1000
    assert 0 < B.frontier_id.size < e.size
    # C: more than 1024 entry tiles, the last one partial; every key is there, no node is created; between 10 % and 90 %
    # of the nodes improve; at least 1000 nodes with the best candidate tied between slices, and the smallest e has won
    assert tiles(Cc.entry_id.size) > SCAN and Cc.entry_id.size % TILE != 0
    assert Cc.n_nodes == B.n_nodes and (Cc.entry_id >= 0).sum() > 4000000
    improved = Cc.g < B.g
    assert 0.1 < improved.mean() < 0.9 and Cc.frontier_id.size == improved.sum()
    assert np.array_equal(Cc.pred[~improved], B.pred[~improved]) and (Cc.pred[improved] >= N_ROWS).all()
    assert nodes_tied_across_slices(sc, snaps, "C") >= 1000
    be, bids = best_entries(sc, snaps, "C")
    first = np.full(Cc.n_nodes, be.size + Cc.entry_id.size, np.int64)
    np.minimum.at(first, bids, be)
    assert np.array_equal(Cc.pred[improved], sc["calls"][2][3][first[improved] // S])
    # the edges: EMPTY as a key in different tiles, rows that do not count, +inf and NaN costs, poisoned tails
    ee = np.array(EMPTY_ENTRIES)
    assert (lists["hash"][ee] == EMPTY).all() and np.unique(ee // TILE).size == ee.size
    assert (Cc.entry_id[ee] >= 0).sum() >= 2 and np.unique(Cc.entry_id[ee][Cc.entry_id[ee] >= 0]).size == 1
    zero = np.nonzero(lists["count"] == 0)[0]
    assert zero.size > 0.005 * N_ROWS and np.isfinite(lists["cost"][zero * S]).sum() > 0.9 * zero.size
    assert (Cc.entry_id.reshape(-1, S)[zero] == -1).all() and (Cc.entry_id.reshape(-1, S)[[7, ROWS_A + 7]] == -1).all()
    assert np.isinf(lists["cost"]).sum() > 10000 and np.isnan(lists["cost"]).sum() > 10000
    k = sc["partial"][0]
    assert np.isnan(lists["cost"][k * S + lists["count"][k]:(k + 1) * S]).all() and lists["count"][k] < S
    # capacities above the final counts: status 0 throughout
    assert Cc.n_nodes < NODE_CAPACITY < 2 ** 31 and Cc.n_nodes - 1 > 2 ** 22


def assert_open_conditions(sc, snaps, goal_hash):
    """What the pushes and selects must contain, on the references alone."""
    A, B, Cc = snaps["A"], snaps["B"], snaps["C"]
    n_tiles = tiles(Cc.n_nodes)
    assert n_tiles > SCAN + 1 and (W_HEUR, V_MAX, TOL) == (OM.HAND_W, OM.HAND_VMAX, OM.HAND_TOL)
    # the bound across the boundary: B's frontier pushed into a table that has just passed 1024 tiles
    opn = open_reference(B, goal_hash)
    opn.push(B.frontier(), ROWS_B * S, 1.0)
    res, sel = opn.select(math.inf, NODE_CAPACITY)
    assert tiles(A.n_nodes) < SCAN < tiles(B.n_nodes) and A.n_nodes + ROWS_B * S > B.n_nodes
    assert res["status"] == OM.SELECTED and res["count"] == B.frontier_id.size > 100000 and res["n_open"] == 0
    assert (sel["id"] < A.n_nodes).sum() > 1000 and (sel["id"] >= SCAN * TILE).sum() > 1000
    # the goal's box: 121 nodes, in at least 3 scan slices, those of the first push too; the goal's own cell has h = 0
    box = np.nonzero(sc["in_box"][key_index_of_nodes(sc, Cc)])[0]
    assert sc["in_box"].sum() == 121 and box.size == 121 and np.unique(scan_slice(box, n_tiles)).size >= 3
    assert (Cc.hash == np.uint64(goal_hash)).sum() == 1
    opn = open_reference(Cc, goal_hash)
    opn.push(Cc.frontier(), N_ROWS * S, 1.0)
    f, fl = opn.arrays()
    flagged = np.nonzero(fl & OM.IS_GOAL)[0]
    assert np.isin(flagged, box).all() and np.unique(scan_slice(flagged, n_tiles)).size >= 3
    assert ((fl & OM.SEEN) > 0).sum() == Cc.frontier_id.size
    for delta, cap in SELECTS:
        was_open = (opn.flags & OM.IS_OPEN) > 0
        res, sel = opn.select(delta, cap)
        assert res["status"] == OM.SELECTED and res["count"] == sel["count"] <= cap
        if (delta, cap) in ((2.5, 16), (80.0, 5000)):  # truncated: a qualifying node with a larger id is still open
            left = np.nonzero((opn.flags & OM.IS_OPEN) > 0)[0]
            assert res["count"] == cap and res["n_open"] > 0
            assert (left[opn.f[left] <= res["f_min"] + delta] > sel["id"][-1]).sum() > 0
        if delta == 80.0:  # (nearly 6000 qualify, the 5000 smallest ids cover most of the 520 slices)
            assert np.unique(scan_slice(sel["id"], n_tiles)).size > 300
        if cap == NODE_CAPACITY:  # rows in more than 1024 tiles' worth of ids, all of them emitted
            assert res["n_open"] == 0 and res["count"] == was_open.sum() > 500000
            assert np.unique(scan_slice(sel["id"], n_tiles)).size > 500
    # the second push: FOUND by the smallest of at least two tied ids in different slices
    p2 = push_two(sc, Cc)
    assert np.unique(p2["id"]).size == p2["count"] and np.isin(box[Cc.hash[box] != np.uint64(goal_hash)], p2["id"]).all()
    opn.push(p2, p2["count"], 1.0)
    res, sel = opn.select(2.5, 5000)
    tied = np.nonzero(((opn.flags & OM.IS_GOAL) > 0) & (opn.f == res["goal_f"]))[0]
    assert res["status"] == OM.FOUND and res["count"] == 0 and res["n_open"] > 100000 and res["goal_f"] == 51.0
    assert tied.size >= 2 and res["goal_id"] == tied.min() and np.unique(scan_slice(tied, n_tiles)).size >= 2
