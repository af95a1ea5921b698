"""CPU: tests/field_model.py, the sequential restatement of include/mplx_field.h, on hand maps and the push rule."""
import numpy as np

import field_model as FM


def grid(rows):
    """rows of '.', '#' as [y][x] -> (blocked [n_cells], dims)"""
    a = np.array([[ch == "#" for ch in r] for r in rows])
    return a.ravel(), [a.shape[1], a.shape[0]]


def at(dist, dims, x, y):
    return int(dist[y * dims[0] + x])


def test_straight_corridor():
    b, dims = grid(["#########",
                    ".........",
                    "#########"])
    d = FM.field(b, dims, [[0, 1]], [[0, 1]])[0]
    assert [at(d, dims, x, 1) for x in range(9)] == list(range(9))
    assert all(at(d, dims, x, y) == -1 for x in range(9) for y in (0, 2))


def test_a_diagonal_gap_is_passable():
    b, dims = grid(["..#..",
                    "..#..",
                    "...#.",
                    "...#."])
    # the wall's two halves touch at a corner only: (2, 1) and (3, 2) are blocked, the step (2, 2) -> (3, 1) is diagonal
    d = FM.field(b, dims, [[0, 0]], [[0, 0]])[0]
    assert at(d, dims, 2, 2) == 2 and at(d, dims, 3, 1) == 3 and at(d, dims, 4, 0) == 4
    assert at(d, dims, 2, 1) == -1 and at(d, dims, 3, 2) == -1


def test_a_sealed_pocket_is_unreachable():
    b, dims = grid([".....",
                    ".###.",
                    ".#.#.",
                    ".###.",
                    "....."])
    d = FM.field(b, dims, [[0, 0]], [[0, 0]])[0]
    assert at(d, dims, 2, 2) == -1 and at(d, dims, 4, 4) == 7 and at(d, dims, 1, 1) == -1   # (4, 4): round the ring


def test_seeds_on_blocked_cells_hold_zero_and_are_sources():
    b, dims = grid(["#####",
                    "##...",
                    "#####"])
    d = FM.field(b, dims, [[0, 0]], [[1, 2]])[0]   # the box covers blocked cells only
    assert all(at(d, dims, x, y) == 0 for x in (0, 1) for y in (0, 1, 2))
    assert [at(d, dims, x, 1) for x in (2, 3, 4)] == [1, 2, 3]   # (2, 1) is reached from the blocked seed (1, 1)
    assert at(d, dims, 2, 0) == -1


def test_clipped_and_outside_boxes():
    b, dims = grid(["....",
                    "....",
                    "...."])
    d = FM.field(b, dims, [[-5, -5], [4, 0], [2, 7]], [[0, 0], [9, 2], [3, 9]])
    assert at(d[0], dims, 0, 0) == 0 and at(d[0], dims, 3, 2) == 3   # clipped to the corner cell
    assert np.all(d[1] == -1) and np.all(d[2] == -1)                 # wholly outside: no seed, all -1
    assert np.array_equal(FM.chebyshev_to_box(dims, [-5, -5], [0, 0]), d[0])


def test_two_fields_on_one_map():
    b, dims = grid([".....",
                    "####.",
                    "....."])
    d = FM.field(b, dims, [[0, 0], [0, 2]], [[0, 0], [0, 2]])
    assert at(d[0], dims, 0, 2) == 8 and at(d[1], dims, 0, 0) == 8
    assert at(d[0], dims, 0, 0) == 0 and at(d[1], dims, 0, 2) == 0
    assert np.array_equal(d[0].reshape(3, 5)[::-1], d[1].reshape(3, 5))


def test_three_dimensions_have_26_neighbours():
    dims = [3, 3, 3]
    b = np.zeros(27, bool)
    d = FM.field(b, dims, [[0, 0, 0]], [[0, 0, 0]])[0]
    assert d[26] == 2 and d[13] == 1
    assert np.array_equal(d, FM.chebyshev_to_box(dims, [0, 0, 0], [0, 0, 0]))


# ---- the push rule
DIMS, ORG, RES = [8, 4], [0.0, 0.0], 0.5
W, VMAX = 10.0, 2.0


def bits(x):
    return np.float64(x).view(np.uint64)


def test_push_rule():
    dist = np.full(32, 7, np.int32)
    goal = [3.75, 0.25]
    pos = [0.25, 0.25]                      # cell (0, 0); L = 3.5
    c = FM.cell_of(pos, DIMS, ORG, RES)
    assert c == 0
    default = FM.default_heuristic(pos, goal, W, VMAX, 2)
    # G <= L: the default's key, bit for bit (n = 8 gives G = 3.5 = L)
    for n in (0, 1, 2, 7, 8):
        dist[c] = n
        h, G, L = FM.heuristic(pos, goal, W, VMAX, dist, DIMS, ORG, RES)
        assert G <= L and bits(h) == bits(default)
        assert bits(FM.key(1.25, 1.0, h)) == bits(FM.key(1.25, 1.0, default))
    # n = 0 and n = 1 give G = 0, so m = L
    for n in (0, 1):
        dist[c] = n
        assert FM.heuristic(pos, goal, W, VMAX, dist, DIMS, ORG, RES)[1] == 0.0
    # G > L
    dist[c] = 20
    h, G, L = FM.heuristic(pos, goal, W, VMAX, dist, DIMS, ORG, RES)
    assert G == 9.5 and L == 3.5 and h == W * 9.5 / VMAX
    # n < 0 and a position off the map: +inf
    dist[c] = -1
    assert np.isinf(FM.heuristic(pos, goal, W, VMAX, dist, DIMS, ORG, RES)[0])
    for off in ([-0.1, 0.25], [4.0, 0.25], [0.25, 2.0], [np.nan, 0.25], [1e300, 0.25]):
        assert FM.cell_of(off, DIMS, ORG, RES) is None
        assert np.isinf(FM.heuristic(off, goal, W, VMAX, np.zeros(32, np.int32), DIMS, ORG, RES)[0])
    assert bits(FM.key(2.0, 1.0, np.inf)) == FM.INF_BITS and FM.key(2.0, 0.0, np.inf) == 2.0
    # the goal's own lattice state keeps h = 0 whatever the field says
    assert FM.heuristic(pos, goal, W, VMAX, dist, DIMS, ORG, RES, is_goal_state=True)[0] == 0.0


def test_float_to_int_is_c_round():
    f = lambda x: FM.float_to_int(x, 0.0, 1.0)
    # (0.0 - 0.5 = -0.5 rounds away from zero: a position exactly on the map's lower edge is outside, as in the reference)
    assert [f(x) for x in (0.0, 0.001, 0.999, 1.0, 1.5, -0.001, -1.0, -1.001)] == [-1, 0, 0, 1, 1, -1, -2, -2]
    assert FM.goal_box([3.75, 0.25], 0.5, ORG, RES) == ([5, -2], [9, 2])
