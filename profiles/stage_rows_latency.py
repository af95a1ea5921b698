"""Wall time of one call of the small host-pointer twins that declare their rows with StageRows (csrc/mplx_stage.h):
the fixed cost of a call is what a change to the staging layer would show in.  n = 16 problems through the C ABI, the
structs filled by the walk helpers of tests/test_gpu_staging_sets.py (visit 0 of each kind: every output row asked
for), mplx_read_cells at n = 1 and 64, and mplx_reserve_check_poly through Reservations.check_poly on the K = B = 65
case of tests/test_gpu_reserve_poly.py.  mplx_shortcut_timed runs the host path of mplx_shortcut.  Median of 300 calls
each, in microseconds, one JSON line; profiles/host_call_latency.py does the same for mplx_expand_lists.

    python profiles/stage_rows_latency.py              # prints {"kind": us, ...}
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402,F401  before libmplx.so is loaded
import motion_primitive_library_amd as m  # noqa: E402
import reserve_poly_cases as RC  # noqa: E402
import staging_walk as SW  # noqa: E402
import test_gpu_reserve_poly as RP  # noqa: E402
import test_gpu_staging_sets as T  # noqa: E402

N, REPS, CONFIG = 16, 300, "3d_acc"
KINDS = ("solve", "poly_load", "poly_info", "poly_sample", "poly_traverse", "poly_limits", "poly_conflicts", "shortcut")


def median_us(fn):
    for _ in range(10):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(float(np.median(ts)) * 1e6, 1)


def main():
    abi, res = m._abi, {}
    w = T.World(CONFIG)
    env = m.EnvMap(w.dim, 0)
    w.configure(env)
    polys = T.Polys(abi, env, N)
    for i, kind in enumerate(KINDS):
        x = w.inputs(i, kind, N, 0)
        I = {k: SW.ptr(x[k]) for k in T.ARRAYS if k in x}
        if x["setter"]:
            T.call(abi, polys, w, x["setter"], N, 0, x, {}, I)
        rows, P = T.host_rows(T.out_spec(w, kind, N, 0, x))
        res[kind] = median_us(lambda: T.call(abi, polys, w, kind, N, 0, x, P, I))
    L = abi.lib()
    for n in (1, 64):
        idx, vals = (np.arange(n, dtype=np.int64) * 7919) % w.cells.size, np.zeros(n, np.int8)
        res["read_cells n=%d" % n] = median_us(lambda: abi.check(env._ctx, L.mplx_read_cells(env._ctx, 0, idx.ctypes.data, n, vals.ctypes.data)))
    polys.free()
    env.close()
    env = RP.make_env(m, 2)
    case = RC.random_case(2, 65, 65)
    poly = RP.load(env, m, case["cand"])
    table, rp = RP.make_table(env, m, case, False)
    res["reserve_check_poly K=65"] = median_us(lambda: table.check_poly(poly, case["t_start"], case["radius"], case["ignore"]))
    for o in (table, rp, poly):
        o.free()
    env.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
