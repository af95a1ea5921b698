"""GPU: the untimed edge pass of the rebase, replan_edge_kernel<D, K, YAW, false> -- what SearchResult.replan launches: no
key fold, no wait rule, the band of the yaw pinning -- for the ten (dim, control) pairs it ran for in no GPU case
(tests/control_matrix.py::UNTIMED_ADDED), on the worlds of tests/test_gpu_timed_replan.py searched untimed.  The rebase is
compared with tests/replan_model.py fed by the CPU oracle on the edited map, exactly; what makes a case worth running (a
bad edge, a kept node below a root, live acc and jerk rows, an edge the heading limit refuses) is asserted on the model
before the device is asked."""
import numpy as np
import pytest

import control_matrix as CM
import replan_model as RM
from test_gpu_replan import cell_index, depths, rebase_both
from test_gpu_timed_replan import controls, world

pytestmark = pytest.mark.gpu

YAW = CM.YAW


def write_state_rows(m, tab, d, rows):
    """Rows `rows` of the states of a download() back into the table."""
    v, n = tab.view(), d["n_nodes"]
    for f in rows:
        row = np.ascontiguousarray(d["state"][f, :n])
        m._abi.check(tab._env._ctx, m._abi.lib().mplx_memcpy_h2d(tab._env._ctx, int(v.state + 8 * f * v.state_stride), row.ctypes.data, row.nbytes))


def good_edges(O, oenv, T, nU):
    """The non-root nodes (roots: the seeds) whose edge holds on the oracle's map, and the edge function."""
    e = RM.OracleEdges(O, oenv, T)
    bad = RM.bad_edges(T, RM.roots_of(T, -1), e, nU)
    return [i for i in sorted(bad) if not bad[i]], bad, e


def poked_rows(m, O, env, tab, d0, oenv, U, row, by, what, without_limit=None):
    """Row `row` of the states of up to three parents of holding edges moved by `by`, nothing else: at least one edge
    that held no longer does, only children of those parents change, and the device drops them as the model says.
    without_limit: the oracle's Env of the same map without the heading limit -- at least one of the edges must be
    refused by the limit alone (finite without it)."""
    nU = len(U)
    T0 = RM.table_from_arrays(d0)
    good, _, _ = good_edges(O, oenv, T0, nU)
    # (for the heading limit: parents of edges that move, a velocity of zero has every heading)
    moves = lambda i: without_limit is None or np.any(U[T0.pred_action[i]][:2] != 0.0)
    parents = sorted(set(T0.pred[i] for i in good if moves(i)))[:3]
    assert parents, what
    d1 = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in d0.items()}
    d1["state"][row, parents] += by
    T1 = RM.table_from_arrays(d1)
    _, bad1, e1 = good_edges(O, oenv, T1, nU)
    flipped = [i for i in good if bad1[i]]
    assert flipped and all(T0.pred[i] in parents for i in flipped), (what, flipped)
    if without_limit is not None:
        free = RM.OracleEdges(O, without_limit, T1)
        refused = [i for i in flipped if e1(T1.pred[i], T1.pred_action[i])[0] != RM.SLOT_FINITE and
                   free(T1.pred[i], T1.pred_action[i])[0] == RM.SLOT_FINITE]
        assert refused, what + ": no edge is refused by the heading limit alone"
    write_state_rows(m, tab, d1, [row])
    fr, _, model, info = rebase_both(m, env, tab, d1, lambda t: RM.OracleEdges(O, oenv, t), nU, what)
    assert all(np.isinf(model.g[i]) for i in flipped) and info["n_bad_edges"] >= len(flipped), what
    print(what, info, "edges that no longer hold", len(flipped))
    fr.free()
    write_state_rows(m, tab, d0, [row])


@pytest.mark.parametrize("dim,control", CM.UNTIMED_ADDED, ids=[CM.untimed_id(*c) for c in CM.UNTIMED_ADDED])
def test_untimed_edges_of_every_pair(engine, oracle_lib, dim, control):
    m, O = engine, oracle_lib
    name = CM.untimed_id(dim, control)
    small = name in CM.UNTIMED_SMALL_U
    j_max, yaw_max = CM.UNTIMED_LIMITS[name]
    K = CM.order_of(control)
    env, grid, dims, oenv_of, cfg = world(m, O, dim, control, small, j_max, yaw_max)
    U = controls(dim, control, small)
    nU, n = len(U), dims[0]
    assert nU == (2 ** (dim + 1) if control & YAW else 3 ** dim)
    # the start stands 0.01 m before the next cell along x: even the slowest controls (0.5 / 24 m) leave the seed's cell with their first edge
    origin = [0.0] * dim
    start = m.Waypoint(dim, control, pos=[n / 2 + 0.99] + [n / 2 + 0.5] * (dim - 1)).to_row()
    goal = m.Waypoint(dim, control, pos=[n - 1.5] * dim).to_row()
    # ---- untimed: no avoid, no time keys.  delta = 0 and the smallest max_rounds with 65 nodes and a node two edges deep
    sr = None
    for rounds in range(1, 400):
        sr = env.search(start, goal, delta=0.0, max_rounds=rounds, capacity=1 << 14, max_frontier=8192, sight=False)
        d0 = sr.table.download()
        T0 = RM.table_from_arrays(d0)
        dep = depths(T0)
        if d0["n_nodes"] >= 65 and max(dep) >= 2:
            break
        assert sr.status == m.search.MAX_ROUNDS, (name, rounds, sr)
        sr.free()
        sr = None
    assert sr is not None and d0["status"] == 0, name
    tab, n0 = sr.table, d0["n_nodes"]
    has_child = set(p for p in T0.pred if p >= 0)
    # ---- the map edit: cells under nodes with children, the deepest first, never the seed's; as many of the first three
    # as leave the model a bad edge and a kept node below the seed
    seed_cell = cell_index(dims, origin, 1.0, start)
    under = []
    for i in sorted([i for i in range(n0) if dep[i] >= 1 and i in has_child], key=lambda i: -dep[i]):
        c = cell_index(dims, origin, 1.0, T0.state[i])
        if c != seed_cell and c not in under:
            under.append(c)
    assert under, name + ": every node with children stands in the seed's cell"
    for k in (3, 2, 1):
        cells = under[:k]
        grid2 = grid.copy()
        grid2[cells] = 100
        oenv = oenv_of(grid2)
        T = RM.table_from_arrays(d0)
        _, info, _ = RM.rebase(T, RM.OracleEdges(O, oenv, T), nU, root=-1)
        if info["n_bad_edges"] >= 1 and info["n_kept"] >= 2:
            break
    env.editMap(cells, 100)
    edges_of = lambda t: RM.OracleEdges(O, oenv, t)
    # ---- what the table must hold for the case to say anything, on the model
    tested = [i for i in range(n0) if T0.pred[i] >= 0]
    if K >= 3:
        assert any(np.any(T0.state[T0.pred[i]][2 * dim:3 * dim] != 0.0) for i in tested), name + ": no live acc row"
    if K == 4:
        assert any(np.any(T0.state[T0.pred[i]][3 * dim:4 * dim] != 0.0) for i in tested), name + ": no live jerk row"
    # a root two edges down, preferably one below which the model keeps a node
    deep = [i for i in range(n0) if dep[i] == 2]
    root2 = deep[0]
    for r in [i for i in deep if i in has_child][:20]:
        T = RM.table_from_arrays(d0)
        _, info, _ = RM.rebase(T, edges_of(T), nU, root=r)
        if info["n_kept"] >= 2:
            root2 = r
            break
    seen = {"bad": False, "kept": False, "dropped": False}
    for root in (-1, root2):
        what = "%s root %d" % (name, root)
        fr, want_fr, model, info = rebase_both(m, env, tab, d0, edges_of, nU, what, root=root, check_edges=True)
        print(what, "nodes", n0, "rounds", rounds, info)
        assert info["n_roots"] == 1, what
        seen["bad"] |= info["n_bad_edges"] >= 1
        seen["kept"] |= info["n_kept"] > info["n_roots"]
        seen["dropped"] |= info["n_kept"] < n0
        if root == -1:
            assert info["n_bad_edges"] >= 1 and info["n_kept"] >= 2, what  # bad edges, and a non-root node is kept
        fr.free()
    assert all(seen.values()), (name, seen)
    if control == (CM.SNP | YAW):
        poked_rows(m, O, env, tab, d0, oenv, U, 3 * dim, 0.1, name + " jerk row moved by one bin")
    if control & YAW and yaw_max > 0:
        # the yaw row of the parents turned by four steps of the yaw controls: the headings stay the lattice's
        more = dict(j_max=j_max) if j_max > 0 else {}
        free = O.Env(dim, control, U, grid2, dims, origin, 1.0, dt=1.0, w=float(env._p.w), wyaw=0.0, v_max=1.0, a_max=1.0, **more)
        poked_rows(m, O, env, tab, d0, oenv, U, 4 * dim, 1.2, name + " yaw row turned by 1.2", without_limit=free)
    sr.free()
    env.close()
