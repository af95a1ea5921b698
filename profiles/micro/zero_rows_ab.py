"""Same-allocation A/B of the zero-row skip (mplx_expand_lists_device_z against mplx_expand_lists_device) on ONE Lists of a
full-size workload: python profiles/micro/zero_rows_ab.py [workload=C4] [rounds=7] [launches=20].

The two placement modes of an allocation (0.48 / 0.555 ms for C4) cannot spoil this comparison: both legs write into the
same buffer, alternately.  The old entry point dirties nothing the mask relies on being zero only because it writes +0.0
there too, but the contract does not let the caller assume that, so the rows are zero-filled again before every masked
leg, outside the timed part."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (spin_up)
import motion_primitive_library_amd as m  # noqa: E402
from motion_primitive_library_amd import _abi  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "C4"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
K = int(sys.argv[3]) if len(sys.argv) > 3 else 20
wl = m.workloads.make(name, potential_fn=m.workloads.device_potential_fn(0) if name == "C5" else None)
env = m.EnvMap(wl.dim, 0)
wl.apply(env)
fr = env.upload_frontier(wl.nodes)
lists = env.alloc_lists(wl.n_nodes, want_state=True, want_iters=False)
L = _abi.lib()


def zero_fill():
    mask = C.c_uint32(0)
    s = lists.c_struct()
    _abi.check(env._ctx, L.mplx_lists_zero_fill(env._ctx, C.byref(s), C.byref(mask)))
    lists.zero_rows = int(mask.value)


def old_entry():
    s = lists.c_struct()
    _abi.check(env._ctx, L.mplx_expand_lists_device(env._ctx, fr.ptr, fr.n_nodes, fr.n_nodes, C.byref(s)))
    lists.zero_rows = 0


def timed(launch):
    for _ in range(3):
        launch()
    env.synchronize()
    env.timer_begin()
    for _ in range(K):
        launch()
    return env.timer_end() / K


spun = bench.spin_up(env, fr, lists)
res = {"mask": [], "old": []}
skipped = None
for r in range(rounds):
    zero_fill()
    env.synchronize()
    res["mask"].append(timed(lambda: env.expand_lists_resident(fr, lists)))
    skipped = env.last_lists_zero_rows()
    res["old"].append(timed(old_entry))
    assert env.last_lists_zero_rows() == 0
    print(json.dumps({"round": r, "mask_ms": round(res["mask"][-1], 4), "old_ms": round(res["old"][-1], 4)}), flush=True)


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


print(json.dumps({
    "workload": name, "kernel": env.last_grid_kernel(), "rows_skipped": "0x%x" % skipped, "spin_up_launches": spun,
    "launches_per_leg": K, "rounds": rounds,
    "mask_ms": {"median": round(med(res["mask"]), 4), "min": round(min(res["mask"]), 4)},
    "old_ms": {"median": round(med(res["old"]), 4), "min": round(min(res["old"]), 4)},
    "ratio_median": round(med(res["mask"]) / med(res["old"]), 4), "ratio_min": round(min(res["mask"]) / min(res["old"]), 4)}))
