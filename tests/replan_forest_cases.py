"""Hand-built forests for the decision passes of the rebase (include/mplx_replan.h: init, resolve, apply, scan, emit of
replan_kernel.hip).  Pure numpy, no GPU and no engine: every case is n nodes with a query column, g, pred and
pred_action, and one or more root settings; all of them are meant for check_edges = 0, so that only the closure over
pred is under test.  tests/test_replan_forest_cases.py holds the cases to the shapes they claim (on the models alone),
tests/test_gpu_replan_forest.py runs them on the device.

Three statements of the rule meet here:
  * replan_model.rebase, the reference of the GPU test (sequential, memoised walks up the chains);
  * kept_by_descent below, written the other way round: from the roots DOWN over the child lists, never up a chain;
  * doubling below, the two buffers of replan_init_kernel / replan_resolve_kernel restated on whole arrays, which says
    after how many passes nothing is UNKNOWN any more (or that a cycle never is).
"""
import math

import numpy as np

import replan_model as RM

TILE = 4096          # ids per workgroup of the apply / emit passes (kTableTile)
N_ACTIONS = 9        # pred_action of a non-root node: any value in [0, N_ACTIONS)
UNKNOWN, KEEP, DROP = 0, 1, 2
CYCLE_LENGTHS = (2, 3, 64, 65, 4097)
TAILS = (1, 70)


def ceil_log2(x):
    p = 0
    while (1 << p) < x:
        p += 1
    return p


def passes_of_bound(bound):
    """ceil(log2(bound)) + 1: the passes the device makes for a table whose node count is at most `bound`."""
    return ceil_log2(max(int(bound), 2)) + 1


class Setting:
    """One call: root (a table of one query) or roots [Q].  want: what the case's shape says about the outcome, any of
    n_roots, n_kept, depth (edges of the deepest kept chain).  cycle: the call leaves a cycle undecided.  capacity: rows
    of the frontier (None: enough)."""

    def __init__(self, name, root=-1, roots=None, want=None, cycle=False, capacity=None):
        self.name, self.root, self.roots, self.want, self.cycle, self.capacity = name, root, roots, dict(want or {}), cycle, capacity

    def args(self):
        return dict(root=self.root, roots=self.roots)


class Case:
    def __init__(self, name, g, pred, settings, query=None, Q=1, family=None, seed=0):
        n = len(pred)
        self.name, self.family, self.n, self.Q = name, family or name, n, Q
        self.g = np.asarray(g, dtype=np.float64)
        self.pred = np.asarray(pred, dtype=np.int32)
        self.query = np.zeros(n, np.int32) if query is None else np.asarray(query, dtype=np.int32)
        rng = np.random.default_rng(1000 + seed)
        self.pred_action = np.where(self.pred >= 0, rng.integers(0, N_ACTIONS, size=n), -1).astype(np.int32)
        self.settings = settings
        assert self.g.shape == self.pred.shape == self.query.shape == (n,)

    def arrays(self, base=None):
        """The case as a download(): its g / pred / pred_action over the hash, state and query of `base` (a download of
        the device table the case was seeded into), or over made-up ones."""
        if base is None:
            base = {"hash": np.arange(1, self.n + 1, dtype=np.uint64), "state": np.arange(self.n, dtype=np.float64)[None, :] * np.ones((2, 1)),
                    "query": self.query, "status": 0}
        d = dict(base)
        d.update(n_nodes=self.n, g=self.g.copy(), pred=self.pred.copy(), pred_action=self.pred_action.copy())
        return d

    def table(self, base=None):
        return RM.table_from_arrays(self.arrays(base), self.Q)


# ------------------------------------------------------------------------------------------ the statements of the rule
def is_root(case, setting):
    """root(id) of the header, on whole arrays."""
    ids = np.arange(case.n)
    r = np.full(case.n, int(setting.root)) if setting.roots is None else np.asarray(setting.roots, dtype=np.int64)[case.query]
    return np.isfinite(case.g) & np.where(r >= 0, ids == r, case.pred == -1)


def bad_without_check(case):
    """With check_edges == 0 the only bad edge is one whose predecessor is no node of the table."""
    return case.pred >= case.n


def kept_by_descent(case, setting):
    """kept(id), from the roots down: a root is kept, and so is every child (pred = a kept node, the child's own edge
    not bad) of a kept node.  A breadth-first walk over the child lists; no chain is ever followed upwards."""
    n = case.n
    root = is_root(case, setting)
    hangs = ~root & (case.pred >= 0) & ~bad_without_check(case)  # the nodes that are kept iff their predecessor is
    order = np.argsort(case.pred[hangs], kind="stable")
    child = np.nonzero(hangs)[0][order]                         # grouped by predecessor
    first = np.searchsorted(case.pred[child], np.arange(n + 1))
    kept = root.copy()
    level = np.nonzero(root)[0]
    while level.size:
        nxt = np.concatenate([child[first[p]:first[p + 1]] for p in level]) if level.size else level
        nxt = nxt[~kept[nxt]]
        kept[nxt] = True
        level = nxt
    return kept


def depth_of_kept(case, setting):
    """Edges of the deepest kept chain below a root (-1: nothing is kept), by the same descent."""
    n = case.n
    root = is_root(case, setting)
    hangs = ~root & (case.pred >= 0) & ~bad_without_check(case)
    order = np.argsort(case.pred[hangs], kind="stable")
    child = np.nonzero(hangs)[0][order]
    first = np.searchsorted(case.pred[child], np.arange(n + 1))
    seen = root.copy()
    level, depth = np.nonzero(root)[0], -1
    while level.size:
        depth += 1
        nxt = np.concatenate([child[first[p]:first[p + 1]] for p in level])
        nxt = nxt[~seen[nxt]]
        seen[nxt] = True
        level = nxt
    return depth


def doubling(case, setting, limit=None):
    """The two buffers of the device on whole arrays: init, then passes that read one buffer and write the other.
    Returns (passes after which nothing is UNKNOWN, or None when a cycle never is; passes after which the UNKNOWN set
    stopped shrinking; the decisions of the last buffer).  limit: more passes than any chain of n nodes can need."""
    n = case.n
    limit = 2 * ceil_log2(max(n, 2)) + 4 if limit is None else limit
    root = is_root(case, setting)
    dec = np.where(root, KEEP, np.where((case.pred < 0) | bad_without_check(case), DROP, UNKNOWN)).astype(np.uint8)
    jump = np.where(dec == UNKNOWN, case.pred, -1).astype(np.int64)
    settled, left = 0, int((dec == UNKNOWN).sum())
    for k in range(1, limit + 1):
        if left == 0:
            break
        new_dec, new_jump = dec.copy(), jump.copy()            # the other buffer
        u = np.nonzero(dec == UNKNOWN)[0]
        j = jump[u]
        dj = dec[j]
        new_dec[u] = dj                                         # adopts a decision, or stays UNKNOWN ...
        new_jump[u] = np.where(dj != UNKNOWN, j, jump[j])       # ... and takes the target's jump
        dec, jump = new_dec, new_jump
        now = int((dec == UNKNOWN).sum())
        if now < left:
            settled, left = k, now
    return (settled if left == 0 else None), settled, dec


# ---------------------------------------------------------------------------------------------------------- the cases
def _chain(order, g_head=0.0):
    """One chain along `order`: order[0] the seed, pred[order[k]] = order[k - 1], g = the distance from the seed."""
    n = len(order)
    pred, g = np.full(n, -1, np.int32), np.zeros(n)
    pred[order[1:]] = order[:-1]
    g[order] = np.arange(n, dtype=np.float64)
    g[order[0]] = g_head
    return g, pred


def _chain_settings(order, middle=True):
    n = len(order)
    out = [Setting("seeds", want=dict(n_roots=1, n_kept=n, depth=n - 1))]
    if middle:  # the node n // 2 edges down the chain: what is above it goes, it and what is below stay
        out.append(Setting("middle", root=int(order[n // 2]), want=dict(n_roots=1, n_kept=n - n // 2, depth=n - 1 - n // 2)))
    return out


def chain_up(n):
    order = np.arange(n)
    g, pred = _chain(order)
    return Case("chain_up-%d" % n, g, pred, _chain_settings(order), family="chain_up", seed=n)


def chain_down(n):
    order = np.arange(n)[::-1]
    g, pred = _chain(order)
    return Case("chain_down-%d" % n, g, pred, _chain_settings(order), family="chain_down", seed=n)


def chain_shuffled(n):
    order = np.random.default_rng(n).permutation(n)
    g, pred = _chain(order)
    return Case("chain_shuffled-%d" % n, g, pred, _chain_settings(order), family="chain_shuffled", seed=n)


def chain_headless(n):
    g, pred = _chain(np.arange(n), g_head=math.inf)
    return Case("chain_headless-%d" % n, g, pred, [Setting("seeds", want=dict(n_roots=0, n_kept=0))], family="chain_headless", seed=n)


def _add_cycle(pred, ids, tails, take):
    """A cycle through `ids` (pred[ids[k]] = ids[k + 1], the last one back to the first) and, per entry of `tails`
    (attachment index, length), a chain of `length` nodes taken from take() that hangs off ids[attachment]."""
    ids = np.asarray(ids)
    pred[ids] = np.roll(ids, -1)
    for at, length in tails:
        up = int(ids[at % len(ids)])
        for _ in range(length):
            i = take()
            pred[i] = up
            up = i


CYCLES_TAIL_PAIRS_65 = 26  # the 65-cycle carries 26 tails of each length, so that a root on it keeps a fifth of the table
CYCLES_SEED_CHAIN = 2300


def cycles():
    """Disjoint cycles of CYCLE_LENGTHS, each with tails of 1 and 70 nodes, laid out in id order: 2, 3, 64, 65 (with
    their tails), then the 4097-cycle from id 2193 on -- it crosses from the first 4096-id tile into the second --, its
    tails, and a seed chain of 2300 nodes that reaches into the third tile."""
    parts = []
    for L in CYCLE_LENGTHS:
        pairs = CYCLES_TAIL_PAIRS_65 if L == 65 else 1
        parts.append((L, [(5 * k + j, t) for k in range(pairs) for j, t in enumerate(TAILS)]))
    n = sum(L + sum(t for _, t in tails) for L, tails in parts) + CYCLES_SEED_CHAIN
    pred, g = np.full(n, -1, np.int32), np.ones(n)
    nxt = [0]

    def take():
        nxt[0] += 1
        return nxt[0] - 1
    where = {}
    for L, tails in parts:
        ids = [take() for _ in range(L)]
        where[L] = ids
        _add_cycle(pred, ids, tails, take)
    chain = np.arange(nxt[0], n)
    pred[chain[1:]] = chain[:-1]
    g[chain] = np.arange(chain.size)
    on65 = int(where[65][7])
    kept65 = 65 + CYCLES_TAIL_PAIRS_65 * sum(TAILS)
    c = Case("cycles", g, pred, [
        Setting("seeds", want=dict(n_roots=1, n_kept=CYCLES_SEED_CHAIN, depth=CYCLES_SEED_CHAIN - 1), cycle=True),
        Setting("on-the-65-cycle", root=on65, want=dict(n_roots=1, n_kept=kept65), cycle=True)], seed=1)
    c.where = where
    return c


FOREST_N = 3 * TILE + 5


def forest(rng_seed=7):
    """Three queries, query[i] = i % 3.  Query 0 is trees only; the cycles of CYCLE_LENGTHS (each with its two tails) run
    through nodes of queries 1 and 2, whose remaining nodes are trees -- the rule never looks at the query of a
    predecessor.  A query's trees are a random recursive forest along a random permutation of its nodes: the first four
    nodes are a chain (so that the fourth, three edges down, has nearly the whole forest below it), every later node
    is a live seed with probability 0.03, a seed with g = +inf with probability 0.015 (of all 12 293 nodes, a third of
    which are on cycles and tails: about 2 % and 1 %), and otherwise hangs below a node drawn from all earlier ones but
    the first three."""
    n, Q = FOREST_N, 3
    rng = np.random.default_rng(rng_seed)
    query = (np.arange(n) % Q).astype(np.int32)
    pred, g = np.full(n, -1, np.int32), np.zeros(n)
    # the last five ids are the fourth tile: 12288 (query 0) goes right below the chain of query 0, 12290 into the 2-cycle
    pool = rng.permutation(np.nonzero((query != 0) & (np.arange(n) != n - 3))[0]).tolist()
    pool.append(n - 3)
    take = pool.pop
    where = {}
    for L in CYCLE_LENGTHS:
        ids = [take() for _ in range(L)]
        where[L] = ids
        _add_cycle(pred, ids, [(0, TAILS[0]), (L // 2, TAILS[1])], take)
    in_cycle = query != 0
    in_cycle[pool] = False
    g[in_cycle] = 5.0
    third, dead = [], []
    for q in range(Q):
        mine = np.nonzero((query == q) & ~in_cycle)[0]
        order = rng.permutation(mine)
        if q == 0:  # n - 5 = 12288 fifth
            order = np.concatenate([order[order != n - 5][:4], [n - 5], order[order != n - 5][4:]])
        depth = np.zeros(n, np.int64)
        for k, i in enumerate(order):
            if k == 0:
                g[i] = 0.0
                continue
            if k < 4:
                p = order[k - 1]
            else:
                u = rng.random()
                if u < 0.045 and not (q == 0 and k == 4):
                    g[i] = 0.0 if u < 0.03 else math.inf
                    if u >= 0.03:
                        dead.append(int(i))
                    continue
                p = order[rng.integers(3, k)]
            pred[i] = p
            depth[i] = depth[p] + 1
            g[i] = float(depth[i])
        third.append(int(order[3]))
    dead1 = next(i for i in dead if query[i] == 1)
    settings = [
        Setting("seeds", roots=[-1, -1, -1], cycle=True),
        Setting("three-edges-down", roots=third, want=dict(n_roots=3), cycle=True),
        # query 0 its seeds; query 1 a seed that was never reached; query 2 a node of query 0, which is kept all the same
        Setting("seeds-none-foreign", roots=[-1, dead1, third[0]], cycle=True),
    ]
    c = Case("forest", g, pred, settings, query=query, Q=Q, seed=2)
    c.where = where
    # once more with a frontier that ends inside the third tile: the rank of the first kept id past 2 * TILE + 2000
    kept = np.nonzero(kept_by_descent(c, settings[0]))[0]
    cut = int(np.searchsorted(kept, 2 * TILE + 2000))
    c.settings.append(Setting("seeds-short", roots=[-1, -1, -1], cycle=True, capacity=cut))
    return c


def pred_out_of_range():
    """Five nodes, one of which names a predecessor that is no node of the table (7 >= n; with the three spare rows of
    the GPU test a row the table owns but does not use): 0 <- 1 <- 4 are kept, 2 (pred 7) and 3 below it are dropped,
    and the edge of 2 is bad whatever check_edges says."""
    g = [0.0, 1.0, 2.0, 3.0, 2.0]
    pred = [-1, 0, 7, 2, 1]
    return Case("pred_out_of_range", g, pred, [Setting("seeds", want=dict(n_roots=1, n_kept=3, depth=2, n_bad_edges=1))], seed=3)


BOUND_N, BOUND_ROWS, BOUND_S = 300, 8, 64


def bound_lists():
    """One seed and BOUND_ROWS lists of BOUND_S entries over 299 distinct hashes, every hash at least once: relaxed
    into a table that holds the seed they make 300 nodes, while the host, which has not waited for the count, has to
    take 1 + 512 for the bound.  Returns (seed state, host lists, parent ids, parent g)."""
    rng = np.random.default_rng(41)
    n_e = BOUND_ROWS * BOUND_S
    pool = rng.choice(np.arange(1000, 100000, dtype=np.uint64), size=BOUND_N - 1, replace=False)
    h = pool[rng.integers(0, pool.size, size=n_e)]
    h[rng.permutation(n_e)[:pool.size]] = pool
    lists = {"stride": BOUND_S, "count": np.full(BOUND_ROWS, BOUND_S, np.int32), "action": (np.arange(n_e) % N_ACTIONS).astype(np.int32),
             "cost": rng.choice([0.5, 1.0, 1.5], size=n_e), "hash": h, "state": rng.standard_normal((10, n_e))}
    return np.zeros(10), lists, np.zeros(BOUND_ROWS, np.int32), np.zeros(BOUND_ROWS)


def bound_above_n():
    """A shuffled chain over the 300 nodes of bound_lists(): 299 edges want 9 passes; the bound 513 gives 11, the node
    count would give 10 -- the last buffer is the other one."""
    order = np.random.default_rng(300).permutation(BOUND_N)
    g, pred = _chain(order)
    return Case("bound_above_n", g, pred, _chain_settings(order, middle=False), seed=4)


CHAIN_UP_SIZES = (2, 3, 5, 64, 65, 257, 4096, 4097, 8193)
_cases = []


def cases():
    if not _cases:
        _cases.extend([chain_up(n) for n in CHAIN_UP_SIZES])
        _cases.extend([chain_down(n) for n in (65, 4097, 8193)])
        _cases.extend([chain_shuffled(n) for n in (4097, 8193)])
        _cases.extend([chain_headless(4097), cycles(), forest(), bound_above_n(), pred_out_of_range()])
    return _cases


def case(name):
    return next(c for c in cases() if c.name == name)


def reference(case, setting, base=None, capacity=None):
    """replan_model.rebase on the case: (table after the call, frontier, result, status)."""
    t = case.table(base)
    fr, res, status = RM.rebase(t, None, 0, check_edges=False, capacity=setting.capacity if capacity is None else capacity, **setting.args())
    return t, fr, res, status
