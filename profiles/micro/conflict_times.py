"""Time of one conflict check between the trajectories of a set (include/mplx_conflict.h) against the only route to the
same answer without it: sample every instant, download, O(K^2 * steps) numpy on the host.

    python profiles/micro/conflict_times.py measure [OUT.json]   # GPU box; default profiles/conflict_times.json

Workload: K = 4096 loaded 3-D trajectories of S = 5 segments (c5 on the quarter grid in [0, 64)^3, c4 in sixteenths within
+-1, c3 within +-0.5, durations quarters in [0.5, 3]), t0 in quarters from -1 to 2, radius 0.25, step 0.25, n_steps = 256,
PARK, no group, no rank.

conflicts: mplx_poly_conflicts_device, first_step / first_partner / min_d2 / status only (no pair matrix).  A timed window
  is CALLS = 5 back-to-back calls between mplx_timer_begin / _end (events on the context's stream) after one untimed call;
  the figure is the window divided by CALLS, the median of REPS = 5 windows.  Also the host-pointer twin by a host clock
  (it ends in a synchronise): what PolyTrajSet.conflicts costs a caller who wants the rows on the host.
host route: PolyTrajSet.sample(times=[n_steps]) on the host form -- all 4D+3 rows of every instant, downloaded, which is
  what the library offered before -- by a host clock, median of 3; then numpy over the pos rows: per instant the K x K
  matrix of d2 in the header's order, d2 < rr^2, the first instant and the minimum per trajectory.  The numpy part is
  timed over NUMPY_STEPS = 16 instants spread over the window (single thread, as numpy runs it) and reported per instant
  and times n_steps: named as the extrapolation it is.
check: at K = 512 of the same workload the device's rows equal tests/conflict_model.py fed with the sampled positions.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, S, D, N_STEPS, STEP, RADIUS = 4096, 5, 3, 256, 0.25, 0.25
REPS, CALLS, NUMPY_STEPS, CHECK_K = 5, 5, 16, 512
JRKxYAW = 0x17


def workload(n=K):
    rng = np.random.default_rng(4242)
    c = np.zeros((S, D + 1, 6, n))
    c[:, :D, 5, :] = rng.integers(0, 256, (S, D, n)) / 4.0
    c[:, :D, 4, :] = rng.integers(-16, 17, (S, D, n)) / 16.0
    c[:, :D, 3, :] = rng.integers(-8, 9, (S, D, n)) / 16.0
    dts = rng.integers(2, 13, (S, n)) / 4.0
    t0 = rng.integers(-4, 9, n) / 4.0
    return c, dts, t0


def numpy_instants(pos, radius, first, dmin, steps):
    """The host's pair pass over the instants `steps` of pos [D][K][n]: updates first [K] and dmin [K] in place."""
    n = pos.shape[1]
    rr2 = (radius + radius) * (radius + radius)
    eye = np.eye(n, dtype=bool)
    for i in steps:
        d2 = None
        for d in range(pos.shape[0]):
            dx = pos[d, :, None, i] - pos[d, None, :, i]
            d2 = dx * dx if d2 is None else d2 + dx * dx
        d2[eye] = np.inf
        hit = (d2 < rr2).any(axis=1) & (first < 0)
        first[hit] = i
        np.minimum(dmin, d2.min(axis=1), out=dmin)


def median(xs):
    return float(np.median(np.asarray(xs)))


def measure(path):
    import motion_primitive_library_amd as m
    import conflict_model as CM
    env = m.EnvMap(D, 0)
    env.set_control(JRKxYAW)
    res = {"trajectories": K, "segments": S, "dim": D, "n_steps": N_STEPS, "step": STEP, "radius": RADIUS, "repetitions": REPS,
           "calls_per_window": CALLS, "device": env.device_info()[0]}

    # ---- check at CHECK_K against the model
    c, dts, t0 = workload(CHECK_K)
    poly = env.load_traj(c, dts, control=JRKxYAW)
    tl = CM.local_times(STEP, N_STEPS, t0, CHECK_K)
    pos = np.ascontiguousarray(poly.sample(times=tl)["samples"][:D].transpose(2, 1, 0))
    want = CM.conflicts(pos, np.ones((N_STEPS, CHECK_K), bool), RADIUS, np.ones(CHECK_K, bool))
    got = poly.conflicts(STEP, N_STEPS, t0=t0, radius=RADIUS, park=True)
    ok = (np.array_equal(got.first_step, want["first_step"]) and np.array_equal(got.partner, want["first_partner"])
          and np.array_equal(got.min_d2.view(np.uint64), want["min_d2"].view(np.uint64)))
    res["check_k"], res["check_equal"] = CHECK_K, bool(ok)
    res["check_share_in_conflict"] = float((want["first_step"] >= 0).mean())
    poly.free()
    if not ok:
        raise SystemExit("conflict_times: the device's rows differ from the model at K = %d" % CHECK_K)

    # ---- the timed workload
    c, dts, t0 = workload(K)
    poly = env.load_traj(c, dts, control=JRKxYAW)
    rows = env.alloc_conflicts(K)
    d_t0 = m.DeviceArray(env, t0.nbytes)
    d_t0.upload(t0)

    def device_call():
        poly.conflicts_resident(rows, STEP, N_STEPS, t0=d_t0, radius=RADIUS, park=True)

    device_call()
    env.synchronize()
    windows = []
    for _ in range(REPS):
        env.timer_begin()
        for _ in range(CALLS):
            device_call()
        windows.append(env.timer_end() / CALLS)
        env.synchronize()
    res["conflicts_device_ms"] = median(windows)
    res["conflicts_device_ms_all"] = windows
    pair_instants = K * (K - 1) / 2 * N_STEPS
    res["pair_instants"] = pair_instants
    res["conflicts_device_pair_instants_per_s"] = pair_instants / (res["conflicts_device_ms"] * 1e-3)

    host = []
    for _ in range(3):
        t = time.perf_counter()
        got = poly.conflicts(STEP, N_STEPS, t0=t0, radius=RADIUS, park=True)
        host.append((time.perf_counter() - t) * 1e3)
    res["conflicts_host_twin_ms"] = median(host)
    res["share_in_conflict"] = float((got.first_step >= 0).mean())

    # ---- the route without it: sample everything, download, numpy
    tl = CM.local_times(STEP, N_STEPS, t0, K)
    out = np.zeros((4 * D + 3, K, N_STEPS))
    samp = []
    for _ in range(3):
        t = time.perf_counter()
        poly.sample(times=tl, out=out)
        samp.append((time.perf_counter() - t) * 1e3)
    res["sample_and_download_ms"] = median(samp)
    res["sample_bytes_downloaded"] = int(out.nbytes)
    steps = [int(x) for x in np.linspace(0, N_STEPS - 1, NUMPY_STEPS)]
    first, dmin = np.full(K, -1, np.int64), np.full(K, np.inf)
    t = time.perf_counter()
    numpy_instants(out[:D], RADIUS, first, dmin, steps)
    per = (time.perf_counter() - t) * 1e3 / len(steps)
    res["numpy_ms_per_instant"] = per
    res["numpy_instants_timed"] = len(steps)
    res["numpy_ms_extrapolated_to_n_steps"] = per * N_STEPS
    res["host_route_ms_extrapolated"] = res["sample_and_download_ms"] + per * N_STEPS
    # the instants the numpy pass did look at agree with the device's minimum from above
    res["numpy_min_not_below_device"] = bool((dmin >= got.min_d2).all())

    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    rows.free()
    d_t0.free()
    poly.free()
    env.close()


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "measure":
        measure(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "conflict_times.json"))
    else:
        raise SystemExit(__doc__)
