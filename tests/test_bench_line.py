"""The ONE JSON line bench.py prints: from a long-form result (a committed bench output of round 5) the compact line
must keep the contract's keys, `roofline`, `cpu_baseline`, the per-configuration numbers, and stay under 8 KB -- a record
that keeps only the tail of stdout must keep all of it (round-5 review: the 30 KB line was cut)."""
import importlib.util
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _long_form():
    path = os.path.join(ROOT, "profiles", "r05_bench_c4_final.json")
    return json.loads([l for l in open(path) if l.startswith("{")][-1])


def test_compact_line_is_small_and_complete():
    b = _bench()
    long_form = _long_form()
    assert len(json.dumps(long_form)) > 16000  # the problem being solved (the driver keeps 8 KB)
    line = b.compact_line(long_form, "bench_detail.json")
    text = json.dumps(line, separators=(",", ":"))
    assert len(text) < 8000, len(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline", "detail"):
        assert k in line, k
    assert line["config"]["workload"].startswith("C4") and "model" not in line["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in line["roofline"], k
    assert abs(line["roofline"]["frac"] - long_form["roofline"]["frac"]) < 1e-5
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    for name in ("C2", "C3", "C5"):
        e = line["other_configs"][name]
        assert e["kernel_ms"] > 0 and "cpu_baseline" in e and "bound" in e and "issue_frac" in e
    assert [c["gpus"] for c in line["strong_scaling_compute_bound"]] == [1, 2, 4, 8]
    assert set(line["plan"]["3D_160"]["engine_host_search"]["timing_split"]) == {"provider_ms", "fill_ms", "pick_ms", "relax_ms", "recover_ms"}
    # numbers only: no prose legs on the line
    def walk(d, path=""):
        for k, v in d.items():
            assert k not in ("what", "timing", "speedup_note"), path + k
            if isinstance(v, dict):
                walk(v, path + k + ".")
    walk(line)


def test_compact_line_survives_failed_legs():
    b = _bench()
    long_form = _long_form()
    long_form["wavefront"] = {"error": "RuntimeError: boom"}
    long_form["other_configs"] = {"error": "x"}
    long_form["plan"]["3D"] = {"error": "y"}
    line = b.compact_line(long_form, "d.json")
    assert line["wavefront"] == {"error": "RuntimeError: boom"} and line["plan"]["3D"] == {"error": "y"}


def test_compact_line_of_a_plain_run():
    """A plain run (no --full) has the headline keys only: no roofline, no legs, no detail file."""
    b = _bench()
    long_form = _long_form()
    plain = {k: long_form[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                       "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")}
    line = b.compact_line(plain, None)
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
    assert abs(line["ms_per_step"] / long_form["ms_per_step"] - 1) < 1e-6 and abs(line["value"] / long_form["value"] - 1) < 1e-6
    assert "roofline" not in line and "detail" not in line and "cpu_baseline" not in line


def test_cpu_baseline_protocol_on_a_small_workload():
    """bench.py::cpu_baseline end to end on the CPU (the reference build or the restatement, whichever is present): the
    repetition is sized by measurement, one warm-up + `reps` timed repetitions, the median and its spread reported, for all
    host threads and for one."""
    import sys
    sys.path.insert(0, ROOT)
    import motion_primitive_library_amd as m
    b = _bench()
    wl = m.workloads.make("C2", scale=0.125, n_nodes=96)
    cb, oenv, n = b.cpu_baseline(wl, rep_seconds=0.08, rep_seconds_1thread=0.05, reps=5)
    assert cb["unit"] == "pairs/s" and cb["value"] > 0 and cb["value_1thread"] > 0
    assert cb["kind"] in ("reference", "port") and "median" in cb["sample"] and cb["cores"] >= 1
    for leg in ("all_cores", "one_thread"):
        p = cb["protocol"][leg]
        assert p["reps"] == 5 and p["min"] <= p["value"] <= p["max"]
        assert p["rep_seconds"] > 0.004, p                         # sized up from the 96-node frontier ...
        assert p["frontier_passes_per_rep"] > 1 and p["frontier_nodes_per_pass"] == 96   # ... by walking it many times
        assert p["nodes_per_rep"] == p["frontier_passes_per_rep"] * 96
    assert n == cb["protocol"]["all_cores"]["nodes_per_rep"] and oenv is not None


class _HostLists:
    """The part of env.Lists that bench.dump_outputs reads, backed by host arrays (nodes x stride entries)."""

    class _Buf:
        def __init__(self, a):
            self.a = a

        def download(self, dtype, shape, offset=0):
            return self.a.view(np.uint8)[offset:].view(dtype)[:int(np.prod(shape))].reshape(shape).copy()

    def __init__(self, n_nodes, stride, n_fields, seed=5):
        rng = np.random.default_rng(seed)
        self.stride, self.n_fields = stride, n_fields
        self.cnt = rng.integers(0, stride + 1, n_nodes).astype(np.int32)
        self.count = self._Buf(self.cnt)
        n = n_nodes * stride
        self.action = rng.integers(0, 1000, n).astype(np.int32)
        self.cost = np.where(rng.random(n) < 0.3, np.inf, rng.random(n))  # (+inf: a blocked successor, as in the lists)
        self.hash = rng.integers(0, 2 ** 63, n, dtype=np.int64).view(np.uint64) | np.uint64(1 << 63)
        self.state = rng.random((n_fields, n))

    def download_nodes(self, lo, hi):
        sl = slice(lo * self.stride, hi * self.stride)
        return {"stride": self.stride, "count": self.cnt[lo:hi].copy(), "action": self.action[sl].copy(),
                "cost": self.cost[sl].copy(), "hash": self.hash[sl].copy(), "state": self.state[:, sl].copy()}


def test_dump_outputs_writes_the_valid_entries_of_a_seeded_sample(tmp_path):
    """--dump-outputs: float64 .npy files, every value finite, every node's count, a sample of nodes fixed by the seed (the
    same in every run), only the entries below each sampled node's count, a blocked successor's +inf cost as blocked = 1
    and cost = 0, the 64-bit hash exact in two halves, and under 64 MB in all."""
    b = _bench()
    lists = _HostLists(1000, 64, 14)
    a, c = str(tmp_path / "a"), str(tmp_path / "c")
    info = b.dump_outputs(lists, 1000, a, node_offset=7)
    b.dump_outputs(lists, 1000, c, node_offset=7)
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    assert sorted(got) == ["action", "blocked", "cost", "count", "hash_hi", "hash_lo", "sample_nodes", "state"]
    assert info["files"] == sorted(f + ".npy" for f in got)
    assert all(v.dtype == np.float64 and np.all(np.isfinite(v)) for v in got.values())
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= 64 * 1024 * 1024
    for f in os.listdir(a):  # the same arguments: the same sample and the same files
        assert np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(c, f)), equal_nan=True)
    assert np.array_equal(got["count"], lists.cnt)
    pick = got["sample_nodes"].astype(np.int64) - 7
    assert pick.size == min(1000, b.DUMP_NODES) and np.all(np.diff(pick) > 0)
    idx = np.concatenate([np.arange(i * 64, i * 64 + lists.cnt[i]) for i in pick])
    assert info["entries"] == idx.size == got["cost"].size
    assert np.array_equal(got["action"], lists.action[idx])
    want = lists.cost[idx]
    assert 0 < got["blocked"].sum() < idx.size and np.array_equal(got["blocked"] == 1.0, np.isinf(want))
    assert np.array_equal(np.where(got["blocked"] == 1.0, np.inf, got["cost"]), want)
    assert np.all(got["cost"][got["blocked"] == 1.0] == 0.0)
    h = (got["hash_hi"].astype(np.uint64) << np.uint64(32)) | got["hash_lo"].astype(np.uint64)
    assert np.array_equal(h, lists.hash[idx])
    assert got["state"].shape == (idx.size, 14) and np.array_equal(got["state"], lists.state[:, idx].T)


def test_dump_outputs_caps_the_sample_at_64_mb(tmp_path):
    b = _bench()
    lists = _HostLists(400, 8192, 14)  # 1.2 MB of entries per node: the byte cap, not DUMP_NODES, sizes the sample
    info = b.dump_outputs(lists, 400, str(tmp_path))
    assert 0 < info["sample_nodes"] < b.DUMP_NODES
    assert sum(os.path.getsize(os.path.join(str(tmp_path), f)) for f in os.listdir(str(tmp_path))) <= 64 * 1024 * 1024
