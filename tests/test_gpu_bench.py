"""GPU: a plain `bench.py` run (no --full) on a small C4 workload: the line carries the headline and nothing else, no detail
file is written, and --dump-outputs writes the lists of the last timed step -- the same files in two runs with the same
arguments, and for the sampled nodes the reference's successors (oracle/_ref, or the restatement where that build is absent)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import oracle_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "C4", "--scale", "0.25", "--nodes", "3000"]


def _plain_run(tmp_path, tag):
    detail = str(tmp_path / ("detail_%s.json" % tag))
    out = str(tmp_path / ("dump_%s" % tag))
    env = dict(os.environ, MPLX_BENCH_DETAIL=detail)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "MPLX_BENCH_FORCE_DIST"):
        env.pop(k, None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", out],
                          cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    assert not os.path.exists(detail)
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}


@pytest.mark.gpu
def test_plain_bench_run_and_its_dumped_outputs(tmp_path, engine, oracle_lib):
    line, dump = _plain_run(tmp_path, "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["value"] == pytest.approx(3000 * 729 / (line["ms_per_step"] * 1e-3), rel=1e-5)
    for k in ("roofline", "cpu_baseline", "parity_sample_ok", "detail", "other_configs", "plan"):
        assert k not in line, k
    assert line["dumped_outputs"]["sample_nodes"] == 256
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in dump.values())
    _, again = _plain_run(tmp_path, "b")
    assert sorted(again) == sorted(dump)
    for k in dump:
        assert np.array_equal(dump[k], again[k], equal_nan=True), k

    # the sampled nodes' successors against the CPU reference
    wl = engine.workloads.make("C4", scale=0.25, n_nodes=3000)
    pick = dump["sample_nodes"].astype(np.int64)
    nU, k = wl.U.shape[0], pick.size
    ref = oracle_lib.expand(oracle_env(wl), np.ascontiguousarray(wl.nodes[:, pick]), threads=8,
                            ref=os.path.exists(oracle_lib.REF_SO))
    cnt = dump["count"].astype(np.int64)[pick]
    slot = np.concatenate([np.arange(i * nU, i * nU + c) for i, c in enumerate(cnt)])
    got = {"stride": nU, "count": cnt.astype(np.int32), "action": np.zeros(k * nU, np.int32), "cost": np.zeros(k * nU),
           "hash": np.zeros(k * nU, np.uint64), "state": np.zeros((dump["state"].shape[1], k * nU))}
    got["action"][slot] = dump["action"].astype(np.int32)
    got["cost"][slot] = np.where(dump["blocked"] == 1.0, np.inf, dump["cost"])  # (blocked: +inf in the lists)
    got["hash"][slot] = (dump["hash_hi"].astype(np.uint64) << np.uint64(32)) | dump["hash_lo"].astype(np.uint64)
    got["state"][:, slot] = dump["state"].T
    from oracle import compare as OC
    assert OC.lists_mismatches(got, ref, k, nU) == []
    assert int(cnt.sum()) > 0 and 0 < int(dump["blocked"].sum()) < int(cnt.sum())
