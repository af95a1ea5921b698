"""Hand cases with known answers for tests/conflict_model.py, the sequential statement of include/mplx_conflict.h that
tests/test_gpu_conflict.py holds the device to.  The robots here move on straight lines at constant speed, so every
expected instant is arithmetic one can do on paper; every coordinate and time is a dyadic rational: no rounding."""
import numpy as np

import conflict_model as CM

STEP = 0.25


def lines(start, vel, total):
    """positions(t0, n, mode) of robots k at start[k] + vel[k] * clamp(tl, 0, total[k])."""
    start, vel, total = np.asarray(start, float), np.asarray(vel, float), np.asarray(total, float)
    K = len(total)

    def positions(t0, n, mode):
        tl = CM.local_times(STEP, n, t0, K)                       # [K][n]
        tc = np.clip(tl, 0.0, total[:, None])
        pos = start[:, None, :] + vel[:, None, :] * tc[:, :, None]  # [K][n][D]
        return np.ascontiguousarray(pos.transpose(1, 0, 2)), CM.active_mask(tl, total, mode)
    return positions


def run(positions, K, n, radius, mode=CM.PARK, t0=None, included=None, **kw):
    pos, act = positions(t0, n, mode)
    inc = np.ones(K, bool) if included is None else included
    return CM.conflicts(pos, act, radius, inc, **kw)


def test_head_on_first_instant():
    # x_a = t, x_b = 10 - t, radii 0.5: distance 10 - 2 t < 1 first at t > 4.5.  i = 18 (t = 4.5) touches: d2 == 1 == rr^2,
    # no conflict; i = 19 (t = 4.75): distance 0.5
    pos = lines([[0, 0], [10, 0]], [[1, 0], [-1, 0]], [10, 10])
    r = run(pos, 2, 41, 0.5)
    assert r["first_step"].tolist() == [19, 19] and r["first_partner"].tolist() == [1, 0]
    assert r["pair_first"].tolist() == [[-1, 19], [19, -1]]
    assert r["min_d2"].tolist() == [0.0, 0.0]  # they meet at t = 5 (i = 20)
    # too few instants to get there: the closest approach so far, no conflict
    r = run(pos, 2, 19, 0.5)
    assert r["first_step"].tolist() == [-1, -1] and r["min_d2"].tolist() == [1.0, 1.0]


def test_touching_is_no_conflict():
    pos = lines([[0, 0, 0], [0, 1, 0]], [[0, 0, 0], [0, 0, 0]], [1, 1])
    r = run(pos, 2, 5, [0.25, 0.75])
    assert r["first_step"].tolist() == [-1, -1] and r["first_partner"].tolist() == [-1, -1]
    assert r["min_d2"].tolist() == [1.0, 1.0] and (r["pair_first"] == -1).all()
    r = run(pos, 2, 5, [0.25, 0.875])  # one sixteenth more: a conflict from the first instant on
    assert r["first_step"].tolist() == [0, 0]


def test_same_group_never_conflicts():
    pos = lines([[0, 0], [0, 0], [0, 0.5]], [[0, 0], [0, 0], [0, 0]], [1, 1, 1])
    r = run(pos, 3, 3, 0.5, group=[7, 7, 9])
    assert r["first_step"].tolist() == [0, 0, 0] and r["first_partner"].tolist() == [2, 2, 0]
    assert r["pair_first"][0, 1] == -1 and r["pair_first"][1, 0] == -1 and r["pair_first"][0, 2] == 0
    assert r["min_d2"].tolist() == [0.25, 0.25, 0.25]  # the pair (0, 1) at distance 0 is no candidate
    r = run(pos, 3, 3, 0.5, group=[7, 7, 7])
    assert r["first_step"].tolist() == [-1, -1, -1] and np.isinf(r["min_d2"]).all()


def test_rank_charging_with_a_tie():
    # three robots on one spot; ranks 0, 1, 1: robot 0 yields to nobody, robots 1 and 2 to 0 and to each other
    pos = lines([[0, 0]] * 3, [[0, 0]] * 3, [1, 1, 1])
    r = run(pos, 3, 2, 0.5, rank=[0, 1, 1])
    assert r["first_step"].tolist() == [-1, 0, 0] and r["first_partner"].tolist() == [-1, 0, 0]
    assert np.isinf(r["min_d2"][0]) and r["min_d2"][1:].tolist() == [0.0, 0.0]
    assert (r["pair_first"] == np.array([[-1, 0, 0], [0, -1, 0], [0, 0, -1]])).all()  # regardless of rank
    # without rank: everybody is charged, the partner is the smallest index
    r = run(pos, 3, 2, 0.5)
    assert r["first_step"].tolist() == [0, 0, 0] and r["first_partner"].tolist() == [1, 0, 0]


def test_park_against_gone_for_a_late_start():
    # robot 0 drives along x through x = 2 at t = 2 and is done at t = 4; robot 1 stands at (2, 0) and starts at t0 = 6
    pos = lines([[0, 0], [2, 0]], [[1, 0], [0, 0]], [4, 1])
    t0 = [0.0, 6.0]
    park = run(pos, 2, 33, 0.25, mode=CM.PARK, t0=t0)
    # |x - 2| < 0.5 first at t = 1.75 (i = 7): at i = 6 the distance is 0.5 exactly
    assert park["first_step"].tolist() == [7, 7] and park["min_d2"].tolist() == [0.0, 0.0]
    gone = run(pos, 2, 33, 0.25, mode=CM.GONE, t0=t0)
    assert gone["first_step"].tolist() == [-1, -1] and np.isinf(gone["min_d2"]).all()  # never active together


def test_excluded_trajectory():
    pos = lines([[0, 0], [0, 0], [0, 0.25]], [[0, 0]] * 3, [1, 1, 1])
    inc = CM.inputs_ok(3, [0.0, np.nan, 0.0], 0.5)
    assert inc.tolist() == [True, False, True]
    assert CM.inputs_ok(3, None, [0.5, -0.5, np.inf]).tolist() == [True, False, False]
    r = run(pos, 3, 2, 0.5, t0=[0.0, np.nan, 0.0], included=inc)
    assert r["first_step"].tolist() == [0, -1, 0] and r["first_partner"].tolist() == [2, -1, 0]
    assert r["min_d2"][1] == np.inf and (r["pair_first"][1] == -1).all() and (r["pair_first"][:, 1] == -1).all()


def crossing():
    """Robot 0 along x, robot 1 along y, both through (4, 4) at tl = 4; 8 s each at speed 1."""
    return lines([[0, 4], [4, 0]], [[1, 0], [0, 1]], [8, 8])


def stagger_positions(lines_fn, total, mode):
    def positions(t0):
        n = CM.n_steps_for(STEP, t0, np.asarray(total, float), np.ones(len(total), bool))
        return lines_fn(t0, n, mode)
    return positions


def test_stagger_resolves_a_crossing():
    # delayed by s, robot 1 is at (4, t - s) while robot 0 is at (t, 4): d2 = (t - 4)^2 + (t - s - 4)^2, least at
    # t = 4 + s / 2 where it is s^2 / 2.  With radii 0.5 a conflict needs d2 < 1.  s = 1: d2 reaches 0.5 (i = 18);
    # s = 2: the minimum is 2.  One delay of 4 * step = 1 is not enough, two are: t0 = [0, 2] after three calls.
    t0, resolved, rounds = CM.stagger(stagger_positions(crossing(), [8, 8], CM.GONE), 2, STEP, 0.5, np.ones(2, bool))
    assert t0.tolist() == [0.0, 2.0] and resolved.tolist() == [True, True] and rounds == 3
    # a larger delay resolves it in one step
    t0, resolved, rounds = CM.stagger(stagger_positions(crossing(), [8, 8], CM.GONE), 2, STEP, 0.5, np.ones(2, bool), delay=2.0)
    assert t0.tolist() == [0.0, 2.0] and resolved.tolist() == [True, True] and rounds == 2
    # equal ranks are both delayed: lockstep, never resolved
    t0, resolved, rounds = CM.stagger(stagger_positions(crossing(), [8, 8], CM.GONE), 2, STEP, 0.5, np.ones(2, bool), rank=[0, 0],
                                      max_rounds=5)
    assert t0.tolist() == [5.0, 5.0] and resolved.tolist() == [False, False] and rounds == 5


def test_stagger_cannot_resolve_a_parked_robot():
    # robot 1 waits at (4, 4) until t0 = 4, the moment robot 0 drives through that point: delaying robot 1 only makes it
    # wait there longer
    pos = lines([[0, 4], [4, 4]], [[1, 0], [0, 1]], [8, 4])
    ok = np.ones(2, bool)
    t0, resolved, rounds = CM.stagger(stagger_positions(pos, [8, 4], CM.PARK), 2, STEP, 0.5, ok, max_rounds=6, t0=[0.0, 4.0])
    assert resolved.tolist() == [True, False] and rounds == 6 and t0.tolist() == [0.0, 10.0]
    # GONE: it does not exist before its start.  Started at t = 5 it appears at (4, 4) with robot 0 at (5, 4): touching,
    # and they part from there
    t0, resolved, rounds = CM.stagger(stagger_positions(pos, [8, 4], CM.GONE), 2, STEP, 0.5, ok, max_rounds=6, t0=[0.0, 4.0])
    assert resolved.tolist() == [True, True] and t0.tolist() == [0.0, 5.0] and rounds == 2
