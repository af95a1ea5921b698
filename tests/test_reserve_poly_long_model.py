"""The inputs of tests/test_gpu_reserve_poly_long.py on the CPU (tests/reserve_poly_cases.py: long_hand_case,
long_random_case, inexact_case, keep_case): the model (tests/reserve_poly_model.py) gives the hits written out by hand,
agrees with its brute force, and the cases have what the device test needs to mean something -- windows past two blocks
of 64 instants, rounded quotients t_start / step, hits whose partner lies past the kKeep = 4 register tiles and that
turn on exclusion and on the ignored group.  No GPU."""
import numpy as np
import pytest

import reserve_poly_cases as RC
import reserve_poly_model as RPM


def run(case, park, brute=False, table=None, ignore="case"):
    c, dts, n_segs = case["cand"]
    rc, rd, rs = case["res"]
    if table is None:
        build = RC.line_table if rc.shape[0] == 1 and not rc[0, :, :5].any() else RC.host_table
        table = build(rc, rd, rs, case["step"], case["n_steps"], case["t0"], case["r_b"], case["group"], park)
    status = np.where(n_segs == 0, 1, 0).astype(np.uint8)
    return RPM.check(status, n_segs, RC.totals(dts, n_segs), case["t_start"], case["radius"],
                     case["ignore"] if isinstance(ignore, str) else ignore, case["step"], table,
                     lambda k, i, tl: RC.segs_position(c, dts, n_segs, k, tl), brute=brute)


def windows(case):
    tot = RC.totals(*case["cand"][1:])
    return [len(RPM.instants(case["step"], case["n_steps"], case["t_start"][k], tot[k])) for k in range(len(tot))]


@pytest.mark.parametrize("park", [False, True])
@pytest.mark.parametrize("D", [2, 3])
def test_long_hand_case(D, park):
    case = RC.long_hand_case(D)
    assert windows(case) == [RC.LONG_ROWS[k][1] for k in range(len(RC.LONG_ROWS))]
    assert sorted(set(windows(case))) == [128, 129, 153, 192, 193, 200]
    hit, status, n_hit = run(case, park)
    assert np.array_equal(hit, case["hit"]), (hit, case["hit"])
    assert not status.any() and n_hit == len(RC.LONG_ROWS) - 1
    assert np.array_equal(run(case, park, brute=True)[0], hit)
    # the table's last instant is somebody's last instant, and the line table is the general one
    k = 13
    assert case["t_start"][k] + case["cand"][1][0, k] == (case["n_steps"] - 1) * case["step"] and hit[k] >> 32 == case["n_steps"] - 1
    rc, rd, rs = case["res"]
    a = RC.line_table(rc, rd, rs, case["step"], 9, case["t0"], case["r_b"], case["group"], park)
    b = RC.host_table(rc, rd, rs, case["step"], 9, case["t0"], case["r_b"], case["group"], park)
    assert all(np.array_equal(a[key], b[key]) for key in b)


@pytest.mark.parametrize("D", [2, 3])
def test_long_random_case(D):
    """At K = B = 65: at least a quarter of the problems have more than 128 instants, between 20 % and 80 % have a hit, some
    leave the horizon, hits lie in the third block of a window and beyond, and the model agrees with its brute force."""
    case = RC.long_random_case(D, 65, 65)
    n = np.array(windows(case))
    hit, _, n_hit = run(case, False)
    first = np.array([int(np.ceil(max(t, 0.0) / case["step"])) for t in case["t_start"]])
    late = int(((hit >= 0) & ((hit >> 32) - first >= 128)).sum())
    print("D=%d: %d of 65 problems with more than 128 instants (the longest %d), share of hits %.3f, %d past the horizon, "
          "%d hits past the second block" % (D, (n > 128).sum(), n.max(), n_hit / 65.0, (hit == -2).sum(), late))
    assert 4 * (n > 128).sum() >= 65 and 0.2 <= n_hit / 65.0 <= 0.8 and (hit == -2).any() and late >= 2
    for K, B in ((1, 1), (1, 65), (65, 1)):
        small = RC.long_random_case(D, K, B)
        for park in (False, True):
            assert np.array_equal(run(small, park)[0], run(small, park, brute=True)[0])
    assert np.array_equal(hit, run(case, False, brute=True)[0])


@pytest.mark.parametrize("step", RC.INEXACT_STEPS)
def test_inexact_case(step):
    """The expected hits follow from the instants; the model finds them, and the kernel's way to find the instants
    (instants_scan) gives the set the header states at every t_start of the case."""
    case = RC.inexact_case(2, step)
    hit, status, n_hit = run(case, False)
    assert np.array_equal(hit, case["hit"]), (hit, case["hit"])
    assert not status.any() and n_hit == (case["hit"] >= 0).sum() and n_hit > len(hit) // 2
    tot = RC.totals(*case["cand"][1:])
    off = 0
    for k, (i, n, j) in enumerate(case["rows"]):
        ts = case["t_start"][k]
        want = RPM.instants(step, case["n_steps"], ts, tot[k])
        assert want.tolist() == ([i, i + 1, i + 2] if n <= 0 else [i + 1, i + 2]), (i, n, want)
        assert np.array_equal(RPM.instants_scan(step, case["n_steps"], ts, tot[k]), want)
        x = np.float64(ts) / np.float64(step)
        off += int(x) != want[0]
    print("step %r: at %d of %d problems floor(t_start / step) is not the first instant" % (step, off, len(hit)))
    assert off >= 10


@pytest.mark.parametrize("B", [320, 513])
@pytest.mark.parametrize("D", [2, 3])
def test_keep_case(D, B):
    """At least 20 problems hit a partner b >= 256 (nobody below 256 is ever met); for at least 5 of them the answer
    changes if the excluded reservations (S = 0, a bad radius) are let in, and for at least 5 if nobody is ignored; the
    last reservation -- at B = 513 the single lane of the last tile -- is somebody's answer."""
    case = RC.keep_case(D, B)
    rc, rd, rs = case["res"]
    table = RC.host_table(rc, rd, rs, case["step"], case["n_steps"], case["t0"], case["r_b"], case["group"], False)
    hit = run(case, False, table=table)[0]
    assert np.array_equal(hit, run(case, False, table=table, brute=True)[0])
    some = hit >= 0
    partner = hit & 0xffffffff
    assert (partner[some] >= 256).all() and some.sum() >= 20
    nobody = case["nobody"]
    by_ignore = int((some & (nobody != hit)).sum()) + int(((hit == -1) & (nobody >= 0)).sum())
    # the excluded let in: they stand (S = 0 has no trajectory: at the origin, where candidates start) with |radius|
    open_table = dict(table, included=np.ones(B, np.uint8), radius=np.where(rs > 0, np.abs(case["r_b"]), 0.25))
    act = np.array(table["active"])
    act[:, table["included"] == 0] = 1
    open_table["active"] = act
    bad = np.nonzero(table["included"] == 0)[0]
    pos = np.array(table["pos"])
    for b in bad[rs[bad] > 0]:  # a bad radius: where its trajectory is
        for i in range(case["n_steps"]):
            tl = min(max(i * case["step"] - case["t0"][b], 0.0), RC.totals(rd, rs)[b])
            pos[i, :, b] = RC.segs_position(rc, rd, rs, b, tl)
    open_table["pos"] = pos
    let_in = run(case, False, table=open_table)[0]
    by_exclusion = int(((hit != -2) & (let_in != hit)).sum())
    print("D=%d B=%d: %d problems hit a partner >= 256, %d answers turn on the ignored group, %d on exclusion, partners %s" % (
        D, B, some.sum(), by_ignore, by_exclusion, sorted(set(partner[some].tolist()))[-3:]))
    assert by_ignore >= 5 and by_exclusion >= 5
    assert (rs[256:] == 0).any() and (case["r_b"][256:] < 0).any()
    k0 = case["rider"]
    assert partner[k0] == B - 1 and hit[k0] >> 32 == int(np.ceil(max(case["t_start"][k0], 0.0) / case["step"]))
