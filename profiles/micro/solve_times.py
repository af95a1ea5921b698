"""Times of the batched trajectory solver (include/mplx_solve.h): K = 4096 problems of W = 17 waypoints in 3-D, smoothing
order 2 (JRK ends), time allocation on the device.

    python profiles/micro/solve_times.py OUT.json [K]

  solve            one mplx_solve_device (waypoints, n_wp and v resident; coefficients, dts, taus written)
  solve_traverse   the same solve and one mplx_poly_traverse_device on a 3-D map of 96^3 cells of 0.25 m (free but one
                   occupied block), v_max = 2: what a caller pays to smooth and check K candidates
  host_dense       tests/solve_model.py solve_dense (the reference's dense method restated in numpy) for HOST_N of the
                   same problems on the host, wall clock; the figure for K problems is that mean times K (stated as an
                   extrapolation: the model is a test oracle in Python, not an optimised host solver)

The device times are the context's timer (events on its stream) around the launches, one warm-up and REPS = 7
repetitions; medians and all samples are reported."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, W, D, HOST_N = 7, 17, 3, 16


def problem_set(K):
    import solve_model as SM
    rng = np.random.default_rng(17)
    wp = np.zeros((4 * D + 2, W, K))
    for k in range(K):
        p = SM.random_path(rng, W, D, step=(0.3, 1.0))
        wp[:D, :, k] = (p - p[0] + rng.uniform(6.0, 18.0, D)).T
    wp[D:3 * D, 0] = np.round(rng.uniform(-0.5, 0.5, (2 * D, K)), 2)
    return wp, np.round(rng.uniform(0.5, 2.0, K), 3)


def main(out_path, K):
    import torch  # noqa: F401  before the library: both then share the HIP runtime
    import motion_primitive_library_amd as m
    import solve_model as SM
    wp, v = problem_set(K)
    env = m.EnvMap(D)
    md = [96, 96, 96]
    grid = np.zeros(md[::-1], np.int8)
    grid[40:56, 40:56, 40:56] = 100
    env.setMap([0.0, 0.0, 0.0], md, grid.ravel(), 0.25)
    env.set_control(m.JRK)
    env.set_v_max(2.0)
    d_wp, d_v = m.DeviceArray(env, wp.nbytes), m.DeviceArray(env, v.nbytes)
    d_wp.upload(wp)
    d_v.upload(v)
    poly = env.alloc_poly(K, W)
    out = env.alloc_solve_out(K, W, m.JRK)
    trav = env.alloc_traj_traverse(K)
    res = {"K": K, "W": W, "D": D, "so": 2, "reps": REPS, "device": env.device_info()}

    def solve():
        env.solve_traj_resident(poly, d_wp, K, W, v_arr=d_v, control=m.JRK, out=out)

    def solve_traverse():
        solve()
        poly.traverse_resident(trav)

    for name, fn in (("solve", solve), ("solve_traverse", solve_traverse)):
        samples = []
        for rep in range(REPS + 1):
            env.synchronize()
            env.timer_begin()
            fn()
            ms = env.timer_end()
            if rep:
                samples.append(ms)
        res[name + "_ms"] = {"median": float(np.median(samples)), "samples": samples}
    env.synchronize()
    assert not poly.status.any()
    t = trav.download()
    res["traverse_inf"] = int(np.isinf(t["cost"]).sum())
    res["traverse_samples"] = int(t["n_samples"].sum())
    flags = SM.path_flags(W, 2)
    t0 = time.perf_counter()
    worst = 0.0
    for k in range(HOST_N):
        vals = np.stack([wp[a * D:(a + 1) * D, :, k].T for a in range(3)])
        dense = SM.solve_dense(vals, flags, SM.allocate_time(wp[:D, :, k].T, v[k]), 2)
        got = poly.coefficients()[:, :, :, k].reshape(-1, D)
        worst = max(worst, float(np.abs(got - dense).max() / np.abs(dense).max()))
    per = (time.perf_counter() - t0) / HOST_N
    res["host_dense_ms_per_problem"] = 1e3 * per
    res["host_dense_ms_extrapolated_to_K"] = 1e3 * per * K
    res["max_rel_diff_device_vs_dense"] = worst
    print(json.dumps(res))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    poly.free()
    for b in (d_wp, d_v):
        b.free()
    trav.free()
    env.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
