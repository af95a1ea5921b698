"""Times of the check of a shortcut's pair set against a reservation table (include/mplx_reserve_poly.h), of the only
route to the same answer without it, and of what the timed shortcut adds to the shortcut.

    python profiles/micro/reserve_poly_times.py measure [OUT.json]   # GPU box; default profiles/reserve_poly_times.json

Workload: Q = 64 chains of W = 60 states (59 random primitives of the nine ACC controls {-0.5, 0, 0.5}^2, dt = 1, from
rest at random cells of a free 256 x 256 map of 1 m cells), full max_hop = 59: P = 64 * 59 * 59 = 222 784 pair problems of
one segment, of which the 64 * 59 * 60 / 2 = 113 280 with j < W are solved.  Reservations: B = 64 and B = 1024 loaded
trajectories of 5 segments in the same area (as profiles/micro/conflict_times.py builds them), t0 in quarters from -1 to
2, radius 0.25, PARK; step 0.25, n_steps = 260 (65 s: every pair ends inside the horizon).  Pair (k, i, j) starts at t_i.

check:   mplx_reserve_check_poly_device on the pair set (hit only).  A window is CALLS = 5 back-to-back calls between
         mplx_timer_begin / _end (events on the context's stream) after one untimed call; the figure is the window over
         CALLS, the median of REPS = 5 windows.
merged:  what the library offered before: the candidates and the reservations loaded into ONE PolyTrajSet and
         conflicts(GONE, want_pairs=True).  The pair matrix of all P + B trajectories would hold 5e10 entries, so the
         candidates go in chunks of CHUNK = 2048 solved pairs, each loaded with the B reservations (EnvMap.load_traj,
         host rows) and checked (PolyTrajSet.conflicts with the pair matrix downloaded, as the answer needs it).  Host
         clock over all chunks, median of 3; and the device part alone (conflicts_resident between events) for one chunk,
         times the number of chunks: named as the extrapolation it is.
shortcut: EnvMap.shortcut_resident on the same device states with and without avoid=, alternating, host clock (each
         ends in a synchronise and reads its rows), median of REPS; the difference is the added cost.
check:   on the first chunk the hits equal min_b (pair_first[k][b] << 32 | b) of the merged route.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

Q, W, N_STEPS, STEP, RADIUS, CHUNK = 64, 60, 260, 0.25, 0.25, 2048
REPS, CALLS = 5, 5


def median(xs):
    return float(np.median(np.asarray(xs)))


def reservations(B):
    rng = np.random.default_rng(4242 + B)
    c = np.zeros((5, 3, 6, B))
    c[:, :2, 5, :] = 96.0 + rng.integers(0, 256, (5, 2, B)) / 4.0
    c[:, :2, 4, :] = rng.integers(-16, 17, (5, 2, B)) / 16.0
    c[:, :2, 3, :] = rng.integers(-8, 9, (5, 2, B)) / 16.0
    return c, rng.integers(2, 13, (5, B)) / 4.0, rng.integers(-4, 9, B) / 4.0


def measure(path):
    import motion_primitive_library_amd as m

    env = m.EnvMap(2)
    env.setMap([0.0, 0.0], [256, 256], np.zeros(256 * 256, np.int8), 1.0)
    env.set_control(m.ACC)
    env.set_u(m.workloads.grid_controls([-0.5, 0.0, 0.5], 2))
    env.set_v_max(3.0)
    env.set_a_max(1.0)
    env.set_dt(1.0)
    rng = np.random.default_rng(7)
    starts = np.zeros((env.n_fields, Q))
    starts[:2] = 96.5 + rng.integers(0, 64, (2, Q))
    actions = rng.integers(0, 9, (W - 1, Q)).astype(np.int32)
    states = np.ascontiguousarray(env.traj_info(starts, actions, want_states=True)["seg_state"])
    d_states = m.DeviceArray(env, states.nbytes)
    d_states.upload(states)
    out = {"Q": Q, "W": W, "max_hop": W - 1, "pairs": Q * (W - 1) * (W - 1), "step": STEP, "n_steps": N_STEPS, "repetitions": REPS,
           "calls_per_window": CALLS, "chunk": CHUNK}

    plain = env.shortcut_resident(d_states, Q, W)
    pairs = plain.pairs
    P = pairs.n
    solved = np.nonzero(pairs.status == 0)[0]
    out["pairs_solved"] = int(len(solved))
    ts = np.repeat(states[-1, :W - 1, :].T.reshape(-1), W - 1)  # t_i of pair (k, i, j), t0 = 0
    d_ts, d_hit = m.DeviceArray(env, ts.nbytes), m.DeviceArray(env, P * 8)
    d_ts.upload(ts)
    seg, dts = pairs.segments()[0], pairs.dts()[0]  # [D + 1][6][P], [P]

    for B in (64, 1024):
        rc, rd, rt0 = reservations(B)
        rp = env.load_traj(rc, rd, control=int(m.ACC))
        table = env.alloc_reservations(rp, STEP, n_steps=N_STEPS, t0=rt0, radius=RADIUS, park=True)
        row = {}
        # ---- the check kernel
        table.check_poly_resident(pairs, d_ts, RADIUS, hit=d_hit)
        env.synchronize()
        win = []
        for _ in range(REPS):
            env.timer_begin()
            for _ in range(CALLS):
                table.check_poly_resident(pairs, d_ts, RADIUS, hit=d_hit)
            win.append(env.timer_end() / CALLS)
        hit = d_hit.download(np.int64, (P,))
        row["check_ms_all"], row["check_ms"] = win, median(win)
        row["pairs_with_a_hit"] = int((hit >= 0).sum())
        # ---- the merged route, chunk by chunk (GONE for the candidates needs a GONE table to compare; the times do not
        # depend on the mode, the comparison below is made against a GONE table)
        gone = env.alloc_reservations(rp, STEP, n_steps=N_STEPS, t0=rt0, radius=RADIUS, park=False)
        want = gone.check_poly(pairs, ts, RADIUS)["hit"]
        chunks = [solved[a:a + CHUNK] for a in range(0, len(solved), CHUNK)]

        def merged_chunk(idx, resident_ms=None):
            n = len(idx)
            c = np.zeros((5, 3, 6, n + B))
            d = np.ones((5, n + B))
            c[0, :, :, :n], d[0, :n] = seg[:, :, idx], dts[idx]
            c[:, :, :, n:], d[:, n:] = rc, rd
            ns = np.concatenate([np.ones(n, np.int32), np.full(B, 5, np.int32)])
            both = env.load_traj(c, d, n_segs=ns, control=int(m.ACC))
            t0 = np.concatenate([ts[idx], rt0])
            grp = np.concatenate([np.zeros(n, np.int32), 1 + np.arange(B, dtype=np.int32)])  # candidates do not meet each other
            res = both.conflicts(STEP, N_STEPS, t0=t0, radius=RADIUS, group=grp, park=False, want_pairs=True)
            if resident_ms is not None:
                rows = env.alloc_conflicts(n + B, want_pairs=True)
                bufs = [m.DeviceArray(env, a.nbytes) for a in (t0, grp)]
                for b_, a in zip(bufs, (t0, grp)):
                    b_.upload(a)
                both.conflicts_resident(rows, STEP, N_STEPS, t0=bufs[0], radius=RADIUS, group=bufs[1], park=False)
                env.synchronize()
                for _ in range(REPS):
                    env.timer_begin()
                    both.conflicts_resident(rows, STEP, N_STEPS, t0=bufs[0], radius=RADIUS, group=bufs[1], park=False)
                    resident_ms.append(env.timer_end())
                for b_ in bufs:
                    b_.free()
                rows.free()
            both.free()
            pf = res.pairs[:n, n:].astype(np.int64)  # the reduction the answer needs: min over b of (first << 32 | b)
            keys = np.where(pf >= 0, (pf << 32) | np.arange(B, dtype=np.int64)[None, :], np.int64(1) << 62).min(axis=1)
            return np.where(keys == np.int64(1) << 62, -1, keys)

        dev = []
        got = merged_chunk(chunks[0], dev)
        assert np.array_equal(got, want[chunks[0]]), "the merged route and the check disagree"
        row["merged_device_ms_one_chunk"], row["merged_chunks"] = median(dev), len(chunks)
        row["merged_device_ms_extrapolated"] = median(dev) * len(chunks)
        walls = []
        for _ in range(3):
            t = time.perf_counter()
            for idx in chunks:
                merged_chunk(idx)
            walls.append((time.perf_counter() - t) * 1e3)
        row["merged_host_route_ms_all"], row["merged_host_route_ms"] = walls, median(walls)
        # ---- what the timed shortcut adds
        a_ms, b_ms = [], []
        for rep in range(REPS + 1):
            t = time.perf_counter()
            s1 = env.shortcut_resident(d_states, Q, W)
            t1 = time.perf_counter()
            s2 = env.shortcut_resident(d_states, Q, W, avoid=table, t0=0.0, radius=RADIUS)
            t2 = time.perf_counter()
            s1.free()
            s2.free()
            if rep:  # (the first pair warms up)
                a_ms.append((t1 - t) * 1e3)
                b_ms.append((t2 - t1) * 1e3)
        row["shortcut_ms"], row["shortcut_avoid_ms"] = median(a_ms), median(b_ms)
        row["shortcut_added_ms"] = median(b_ms) - median(a_ms)
        row["shortcut_ms_all"], row["shortcut_avoid_ms_all"] = a_ms, b_ms
        out["B%d" % B] = row
        print("B = %d: check %.3f ms; merged route %.1f ms (device part, extrapolated: %.1f ms); shortcut %.1f ms, with avoid %.1f ms"
              % (B, row["check_ms"], row["merged_host_route_ms"], row["merged_device_ms_extrapolated"], row["shortcut_ms"],
                 row["shortcut_avoid_ms"]), flush=True)
        for x in (gone, table, rp):
            x.free()
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "reserve_poly_times.json"))
    else:
        print(__doc__)
