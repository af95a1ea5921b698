"""Times of the batched rollout call (include/mplx_rollout.h) at user size, against the only way to answer the same
question without it: H dense expansions of the K current states with a gather of the chosen slot in between.

    python profiles/micro/rollout_times.py measure OUT.json   # device-event and wall times (GPU box)
    python profiles/micro/rollout_times.py trace [CASE]       # one rollout call per case, for a kernel trace or a counter
                                                              # run of its own:
        rocprofv3 --kernel-trace --stats -d DIR -o r -- python profiles/micro/rollout_times.py trace
        rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU -d DIR -o c -- python profiles/micro/rollout_times.py trace C4

Cases: C4's map (512^3) and controls (|U| = 729) with (a) K distinct at-rest starts (the frontier's positions) and (b)
one start; C2 and C5 (potential map made on the device) as the 2D and the yaw / potential cases.  K = 65 536, H = 8.
Actions are "guided" (tests/rollout_model.py) with the ENGINE's dense expansion as the judge: random length 1..H, each
step with probability 0.9 a random action the dense kernel finds FINITE from the state reached, else a uniform one.

measure: one warm-up, 7 repetitions, median.  `rollout_ms`: mplx_rollout_device between mplx_timer_begin /
_end (events on the context's stream).  The chained form alternates with it in the same process: per step one
mplx_expand_device on the K current states (K x |U| pairs, status / cost / state rows) -- `chain_expand_ms`, the sum of
the H launches under the same events -- and a gather of slot (k, a_h[k]) into the next states with torch indexing on the
output buffers; `chain_wall_ms` is the wall clock of the whole chain with its synchronisations, `rollout_wall_ms` the
wall clock of the rollout call with its own.  mplx_expand_device is untouched by the rollout feature, so the chain is
what the commit before it can do.
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

K, H, REPS, SEED, P = 65536, 8, 7, 11, 0.9
CASES = ["C4", "C4-one-start", "C2", "C5"]


def setup(case):
    import motion_primitive_library_amd as m
    name = case.split("-")[0]
    wl = m.workloads.make(name, n_nodes=K, potential_fn=m.workloads.device_potential_fn(0) if name == "C5" else None)
    env = m.EnvMap(wl.dim, 0)
    wl.apply(env)
    env._flush()
    starts = wl.nodes.copy()
    starts[wl.dim:, :] = 0.0
    if case.endswith("one-start"):
        starts = np.repeat(starts[:, :1], K, axis=1)
    return m, wl, env, starts


class Chain:
    """H dense expansions with the gather of the chosen slot between them, everything resident (torch-owned buffers)."""

    def __init__(self, m, env, wl):
        import torch
        from motion_primitive_library_amd.shard import TorchArray
        self.m, self.env, self.torch = m, env, torch
        self.nU, self.F = wl.U.shape[0], 4 * wl.dim + 2
        n = K * self.nU
        self.nodes = TorchArray(self.F * K * 8, "cuda:0")
        self.status, self.cost = TorchArray(n, "cuda:0"), TorchArray(n * 8, "cuda:0")
        self.state = TorchArray(self.F * n * 8, "cuda:0")
        self.succ = m._abi.Succ()
        self.succ.status, self.succ.cost, self.succ.state, self.succ.state_stride = self.status.ptr, self.cost.ptr, self.state.ptr, n
        self.base = torch.arange(K, device="cuda:0", dtype=torch.int64) * self.nU

    def views(self):
        t = self.torch
        n = K * self.nU
        return (self.nodes.view(t.float64, self.F * K).view(self.F, K), self.status.view(t.uint8, n), self.cost.view(t.float64, n),
                self.state.view(t.float64, self.F * n).view(self.F, n))

    def expand(self):
        L = self.m._abi.lib()
        self.m._abi.check(self.env._ctx, L.mplx_expand_device(self.env._ctx, self.nodes.ptr, K, K, C.byref(self.succ)))

    def run(self, starts_t, actions_t, timed=False):
        """Walks all K sequences; returns (status, steps, prefix) tensors and the summed event time of the launches."""
        t = self.torch
        nodes, status, cost, state = self.views()
        nodes.copy_(starts_t)
        t.cuda.synchronize()
        alive = t.ones(K, dtype=t.bool, device="cuda:0")
        st_out = t.ones(K, dtype=t.uint8, device="cuda:0")
        steps = t.zeros(K, dtype=t.int32, device="cuda:0")
        prefix = t.zeros(K, dtype=t.float64, device="cuda:0")
        ev_ms = 0.0
        for h in range(H):
            a = actions_t[h].to(t.int64)
            alive &= a >= 0
            if timed:
                self.env.timer_begin()
            self.expand()
            if timed:
                ev_ms += self.env.timer_end()
            self.env.synchronize()
            slot = self.base + a.clamp(min=0)
            s = status[slot]
            ok = alive & (s == 1)
            st_out = t.where(alive & ~ok, s, st_out)
            prefix = t.where(ok, prefix + cost[slot], prefix)
            steps += ok.to(t.int32)
            nodes.copy_(t.where(ok[None, :], state[:, slot], nodes))
            alive = ok
            t.cuda.synchronize()
        return st_out, steps, prefix, ev_ms

    def guided(self, starts_t, rng):
        """Action sequences judged by the engine's own dense expansion (cf. tests/rollout_model.guided)."""
        t = self.torch
        nodes, status, cost, state = self.views()
        nodes.copy_(starts_t)
        t.cuda.synchronize()
        lens = t.from_numpy(rng.integers(1, H + 1, size=K)).to("cuda:0")
        actions = t.from_numpy(rng.integers(0, self.nU, size=(H, K)).astype(np.int32)).to("cuda:0")
        alive = t.ones(K, dtype=t.bool, device="cuda:0")
        gen = t.Generator(device="cuda:0")
        gen.manual_seed(SEED)
        for h in range(H):
            alive &= lens > h
            self.expand()
            self.env.synchronize()
            fin = status.view(K, self.nU) == 1
            best = (t.rand((K, self.nU), device="cuda:0", generator=gen) * fin).argmax(1)
            use = (t.rand(K, device="cuda:0", generator=gen) < P) & fin.any(1)
            a = t.where(use, best, actions[h].to(t.int64))
            actions[h] = a.to(t.int32)
            slot = self.base + a
            ok = alive & (status[slot] == 1)
            nodes.copy_(t.where(ok[None, :], state[:, slot], nodes))
            alive = ok
            t.cuda.synchronize()
        for h in range(H):
            actions[h][lens <= h] = -1
        t.cuda.synchronize()
        return actions


def live_lane_share(status, steps):
    """Pairs evaluated over lane-steps executed: a wave walks until its last lane stops (no re-packing)."""
    evals = steps + np.isin(status, (0, 2, 3))  # a stopped rollout evaluated the pair that stopped it
    waves = evals.reshape(-1, 64)
    return float(evals.sum() / (64.0 * waves.max(axis=1).sum())), int(evals.sum())


def measure(path):
    import torch
    res = {"K": K, "H": H, "repetitions": REPS, "cases": {}}
    for case in CASES:
        m, wl, env, starts = setup(case)
        res["device"] = env.device_info()[0]
        ch = Chain(m, env, wl)
        starts_t = torch.from_numpy(starts).to("cuda:0")
        actions_t = ch.guided(starts_t, np.random.default_rng(SEED))
        one = case.endswith("one-start")
        d_starts = env.upload_frontier(starts[:, :1] if one else starts)
        out = env.alloc_rollouts(K)
        roll_ms, roll_wall, chain_ms, chain_wall = [], [], [], []
        for r in range(REPS + 1):  # the first is the warm-up; the two forms alternate
            t0 = time.perf_counter()
            env.timer_begin()
            env.rollout_resident(d_starts, actions_t, out, H, n_starts=1 if one else K, start_stride=1 if one else K)
            ms = env.timer_end()
            env.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            c_status, c_steps, c_prefix, ev = ch.run(starts_t, actions_t, timed=True)
            cw = (time.perf_counter() - t0) * 1e3
            if r:
                roll_ms.append(ms); roll_wall.append(w); chain_ms.append(ev); chain_wall.append(cw)
        got = out.download()
        status = got["status"] & 0x7f
        # the two forms answer the same question: same status, steps and prefix cost (same device arithmetic)
        agree = bool(np.array_equal(status, c_status.cpu().numpy()) and np.array_equal(got["steps"], c_steps.cpu().numpy())
                     and np.array_equal(got["prefix_cost"], c_prefix.cpu().numpy()))
        share, pairs = live_lane_share(status, got["steps"])
        rm = float(np.median(roll_ms))
        res["cases"][case] = {
            "nU": int(wl.U.shape[0]), "map_dim": wl.map_dim, "rollout_ms": rm, "rollout_ms_all": roll_ms,
            "rollout_wall_ms": float(np.median(roll_wall)), "chain_expand_ms": float(np.median(chain_ms)),
            "chain_wall_ms": float(np.median(chain_wall)), "chain_pairs": int(K) * int(wl.U.shape[0]) * H,
            "pairs_evaluated": pairs, "pairs_per_s": pairs / (rm * 1e-3), "live_lane_share": share,
            "mean_steps": float(got["steps"].mean()), "heading_band_rollouts": int((got["status"] & 0x80 != 0).sum()),
            "shares_same_complete_blocked_dyn": [float((status == s).mean()) for s in range(4)],
            "chain_agrees": agree, "speedup_vs_chain_expand": float(np.median(chain_ms)) / rm}
        print(case, json.dumps(res["cases"][case]), flush=True)
        env.close()
        del ch
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        json.dump(res, f, indent=1)


def trace(cases):
    import torch
    for case in cases:
        m, wl, env, starts = setup(case)
        ch = Chain(m, env, wl)
        starts_t = torch.from_numpy(starts).to("cuda:0")
        actions_t = ch.guided(starts_t, np.random.default_rng(SEED))
        one = case.endswith("one-start")
        d_starts = env.upload_frontier(starts[:, :1] if one else starts)
        out = env.alloc_rollouts(K)
        for _ in range(3):
            env.rollout_resident(d_starts, actions_t, out, H, n_starts=1 if one else K, start_stride=1 if one else K)
            env.synchronize()
        print("trace ok:", case, "mean steps %.2f" % out.download()["steps"].mean(), flush=True)
        env.close()


if __name__ == "__main__":
    cmd = sys.argv[1] if len(sys.argv) > 1 else "measure"
    if cmd == "measure":
        measure(sys.argv[2])
    elif cmd == "trace":
        trace(sys.argv[2:] or CASES)
    else:
        raise SystemExit(__doc__)
