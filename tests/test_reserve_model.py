"""Hand cases for tests/reserve_model.py, the sequential restatement of include/mplx_reserve.h and of the time keys of
include/mplx_table.h.  No GPU: the device side is held against the same model in tests/test_gpu_reserve.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reserve_model as rm  # noqa: E402

INF = np.inf


def table(pos_fn, n_steps, step, B, D=2, active=None, radius=0.5, group=None, included=None):
    """A reservation table from closed forms: pos_fn(b, t) -> [D]."""
    pos = np.zeros((n_steps, D, B))
    for i in range(n_steps):
        for b in range(B):
            pos[i, :, b] = pos_fn(b, np.float64(i) * np.float64(step))
    return {"pos": pos, "active": np.ones((n_steps, B), np.uint8) if active is None else np.asarray(active, np.uint8),
            "included": np.ones(B, np.uint8) if included is None else np.asarray(included, np.uint8),
            "radius": np.broadcast_to(np.float64(radius), (B,)).copy(),
            "group": np.arange(B, dtype=np.int32) if group is None else np.asarray(group, np.int32)}


def vel_chain(x0, u, dt, n):
    """n edges of a VEL robot along x from x0 with input u: one list row per edge, one entry each (S = 1)."""
    parent_t = np.arange(n) * np.float64(dt)
    px = x0 + u * parent_t

    def edge_pos(k, j, i, s):
        return rm.primitive_pos([px[k], 0.0], [0, 0], [0, 0], [0, 0], [u, 0.0], 1, s)
    return parent_t, edge_pos


def run(parent_t, edge_pos, res, step, dt=1.0, t0=0.0, radius=0.5, ignore=-1, cost=None, count=None, parent_id=None):
    n = len(parent_t)
    n_steps = res["pos"].shape[0]
    return rm.check(np.ones(n, np.int32) if count is None else count, np.zeros(n, np.int32),
                    np.ones(n) if cost is None else cost, 1, np.zeros(n, np.int32) if parent_id is None else parent_id,
                    parent_t, dt, 1, step, n_steps, res, ([t0], [radius], [ignore]), edge_pos)


def test_head_on_first_instant():
    # a: x = t, b: x = 10 - t, radii 0.5 + 0.5: |2 t - 10| < 1 first holds at t = 4.75 on a clock of 0.25: instant 19
    res = table(lambda b, t: [10.0 - t, 0.0], 64, 0.25, 1)
    parent_t, edge_pos = vel_chain(0.0, 1.0, 1.0, 8)
    out, hit, nb, looked = run(parent_t, edge_pos, res, 0.25)
    assert looked.all()
    assert hit.tolist() == [-1, -1, -1, -1, (19 << 32) | 0, (20 << 32) | 0, -1, -1]
    assert np.array_equal(np.isinf(out), hit != -1) and nb == 2
    # instant 20 (t = 5) is the boundary of edges 4 and 5: edge 5 is blocked AT it, edge 4 before it
    assert hit[5] >> 32 == 20 and 20 in rm.instants(0.25, 64, 0.0, 4.0, 5.0) and 20 in rm.instants(0.25, 64, 0.0, 5.0, 6.0)


def test_touching_is_not_blocked():
    # b stands at x = 5, y = 1; a passes along y = 0: the closest approach is d = 1 = rr exactly, at t = 5
    res = table(lambda b, t: [5.0, 1.0], 64, 0.25, 1)
    parent_t, edge_pos = vel_chain(0.0, 1.0, 1.0, 8)
    out, hit, nb, _ = run(parent_t, edge_pos, res, 0.25)
    assert (hit == -1).all() and nb == 0 and np.isfinite(out).all()
    # a hair's breadth closer and the two edges that share t = 5 are both blocked, at their shared instant
    res = table(lambda b, t: [5.0, np.nextafter(1.0, 0.0)], 64, 0.25, 1)
    out, hit, nb, _ = run(parent_t, edge_pos, res, 0.25)
    assert hit.tolist() == [-1, -1, -1, -1, 20 << 32, 20 << 32, -1, -1] and nb == 2


def test_ignore_group_and_excluded():
    res = table(lambda b, t: [10.0 - t, 0.0], 64, 0.25, 3, group=[7, 7, 9], included=[1, 0, 1])
    parent_t, edge_pos = vel_chain(0.0, 1.0, 1.0, 8)
    _, hit, _, _ = run(parent_t, edge_pos, res, 0.25)
    assert hit[4] == (19 << 32) | 0
    _, hit, _, _ = run(parent_t, edge_pos, res, 0.25, ignore=7)
    assert hit[4] == (19 << 32) | 2  # group 7 is skipped, b = 1 is excluded anyway
    res["included"][2] = 0
    _, hit, nb, _ = run(parent_t, edge_pos, res, 0.25, ignore=7)
    assert (hit == -1).all() and nb == 0


def test_gone_is_inactive_before_its_t0():
    # b stands at x = 2 and starts at t0 = 2.5 on the clock; the robot (x = t) is inside rr = 1 for t in (1, 3)
    import conflict_model as cm
    tl = cm.local_times(0.25, 64, [2.5], 1)
    parent_t, edge_pos = vel_chain(0.0, 1.0, 1.0, 8)
    park = table(lambda b, t: [2.0, 0.0], 64, 0.25, 1, active=cm.active_mask(tl, [100.0], cm.PARK))
    gone = table(lambda b, t: [2.0, 0.0], 64, 0.25, 1, active=cm.active_mask(tl, [100.0], cm.GONE))
    _, hit, _, _ = run(parent_t, edge_pos, park, 0.25)
    assert hit.tolist()[:4] == [-1, 5 << 32, 8 << 32, -1]  # t = 1 and t = 3 are touching
    _, hit, _, _ = run(parent_t, edge_pos, gone, 0.25)
    assert hit.tolist()[:4] == [-1, -1, 10 << 32, -1]  # b exists from instant 10 (t = 2.5) on


def test_horizon():
    res = table(lambda b, t: [100.0, 100.0], 13, 0.25, 1)  # instants up to t = 3
    parent_t, edge_pos = vel_chain(0.0, 1.0, 1.0, 5)
    out, hit, nb, _ = run(parent_t, edge_pos, res, 0.25)
    assert hit.tolist() == [-1, -1, -1, -2, -2] and nb == 2 and np.isinf(out[3:]).all()
    # a start later on the clock moves the horizon with it
    _, hit, _, _ = run(parent_t, edge_pos, res, 0.25, t0=1.5)
    assert hit.tolist() == [-1, -2, -2, -2, -2]
    # entries that are not looked at stay -1 even past the horizon
    _, hit, nb, looked = run(parent_t, edge_pos, res, 0.25, cost=np.array([1, 1, 1, INF, 1.0]), parent_id=np.array([0, 0, 0, 0, -1]))
    assert hit.tolist() == [-1, -1, -1, -1, -1] and nb == 0 and looked.tolist() == [True, True, True, False, False]


def test_step_that_does_not_divide_dt():
    assert rm.instants(0.3, 100, 0.0, 1.0, 2.0).tolist() == [4, 5, 6]
    assert rm.instants(0.3, 100, 0.0, 2.0, 3.0).tolist() == [7, 8, 9, 10]  # 10 * 0.3 == 3.0 in doubles
    assert rm.instants(0.3, 100, 0.0, 3.0, 4.0).tolist() == [10, 11, 12, 13]
    res = table(lambda b, t: [10.0 - t, 0.0], 100, 0.3, 1)
    parent_t, edge_pos = vel_chain(0.0, 1.0, 1.0, 8)
    _, hit, _, _ = run(parent_t, edge_pos, res, 0.3)
    # |2 t - 10| < 1 for t in (4.5, 5.5): instants 16 (4.8), 17 (5.1), 18 (5.4)
    assert hit.tolist() == [-1, -1, -1, -1, 16 << 32, 17 << 32, -1, -1]


def test_scan_finds_the_stated_set():
    rng = np.random.default_rng(5)
    for _ in range(3000):
        step = float(rng.choice([0.25, 0.3, 0.1, 1.0 / 3.0, 0.7, 1.7]))
        dt = float(rng.choice([1.0, 0.5, 0.25, 0.3]))
        t0 = float(rng.choice([0.0, 0.3, 2.0, 1e-9, 7.1]))
        tp = np.float64(rng.integers(0, 40)) * np.float64(dt) if rng.random() < 0.8 else np.float64(rng.random() * 30)
        tc = tp + np.float64(dt)
        n_steps = int(rng.integers(1, 200))
        assert rm.instants_scan(step, n_steps, t0, tp, tc, dt).tolist() == rm.instants(step, n_steps, t0, tp, tc).tolist()


def test_time_key_fold():
    # std::round is half away from zero: 0.05 / 0.1 = 0.5 -> 1, -0.05 -> -1, 0.25 / 0.1 = 2.5 -> 3 (Python's round: 2)
    assert rm.round_half_away(0.5) == 1 and rm.round_half_away(-0.5) == -1 and rm.round_half_away(2.5) == 3
    assert rm.round_half_away(0.49999999999999994) == 0 and rm.round_half_away(-2.4) == -2 and rm.round_half_away(7.0) == 7
    assert np.float64(0.05) / np.float64(0.1) == 0.5
    # combine(h, v) = h ^ (v + 0x9e3779b9 + (h << 6) + (h >> 2)) in 64 bits, v sign-extended
    assert rm.hash_combine(0, 0) == 0x9E3779B9
    assert rm.hash_combine(0, 1) == 0x9E3779BA
    assert rm.hash_combine(0, -1) == 0x9E3779B8  # 2^64 - 1 + 0x9e3779b9 wraps
    assert rm.hash_combine(1, -1) == 1 ^ ((0xFFFFFFFFFFFFFFFF + 0x9E3779B9 + 64 + 0) & rm.MASK)
    h = 0x0123456789ABCDEF
    assert rm.time_key(h, 0.05) == rm.hash_combine(h, 1)
    assert rm.time_key(h, -0.05) == rm.hash_combine(h, -1)
    assert rm.time_key(h, 0.0) == rm.hash_combine(h, 0)
    assert rm.time_key(h, 12.3) == rm.hash_combine(h, 123)
    assert rm.time_key(h, -0.7) == rm.hash_combine(h, -7)
    assert rm.time_key(h, 0.3) != rm.time_key(h, 0.4) and rm.time_key(h, 0.3) != h


# ---- the header itself
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_function_of_the_header_is_declared_in_abi(engine):
    import re
    text = open(os.path.join(ROOT, "include", "mplx_reserve.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(mplx_[a-z0-9_]+)\s*\(", text)))
    assert "mplx_reserve_check_device" in syms and sorted(engine._abi.RESERVE_SYMBOLS) == syms
    lib = engine._abi.lib()
    for s in syms:
        assert getattr(lib, s).argtypes is not None, s
    assert engine._abi.RESERVE_MAX_BYTES == 1 << 30 and "MPLX_RESERVE_MAX_BYTES = 1 << 30" in text


def test_header_parses_as_c():
    import subprocess
    for h in ("mplx_reserve.h", "mplx_table.h"):
        r = subprocess.run(["gcc", "-fsyntax-only", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "include", h)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


def test_host_fold_is_the_models(engine):
    """mplx_time_key (std::round in the library's host code) against the model, the half cases and negatives included."""
    h = np.array([0, 1, 0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15], np.uint64)
    for t in (0.0, 0.05, -0.05, 0.15, 0.25, 0.3, 0.04, 12.3, -0.7, -1.25, 99.95):
        got = engine.search.time_key(h, t)
        assert got.tolist() == [rm.time_key(int(x), t) for x in h], t
