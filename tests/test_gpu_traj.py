"""Trajectory<Dim> on the device (include/mplx_traj.h, csrc/traj_kernel.hip) against the numpy model
(tests/traj_model.py, pinned on the CPU to the reference's own Trajectory and env_map::traverse_trajectory by
tests/test_traj.py): every row of every call bit for bit, no sample and no trajectory left out, no tolerance; every
lanes-per-trajectory instantiation of the traversal; strides with sentinels; the map as edited on the device; the
resident forms and torch tensors; argument and state errors; the rest of the context untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before libmplx.so is loaded: the library then binds to the HIP runtime torch brought, and a
#               tensor and an engine context can share the device whichever of the two opens it first

import traj_model as M

K = M.GPU_K          # 193: not a multiple of 64
H = M.HORIZON        # 5, S from 0 to 5
N_UNIFORM = 70       # 71 samples: not a multiple of 4, 16 or 64
DT = 0.7
SENTINEL = -7.25e77
LANES = [0, 4, 16, 64]
V_MAXES = [0.3, 2.0, 21.0]  # n + 1 from 2 (0.3 * 0.7 / 0.25 -> 1) to 295 (21 * 3.5 / 0.25 -> 294)
CASES = [(c, d) for d in (2, 3) for c in M.CONTROLS]
IDS = ["c%02x-%dD" % c for c in CASES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.shape[0] == 0, "%s: %d entries differ, first at %s: got %r want %r" % (
        what, bad.shape[0], bad[0].tolist(), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def world(control, dim):
    """(U, starts, actions, geo, grid, pot, trajs of the model), computed once and never changed."""
    U, starts, actions, geo, grid, pot = M.gpu_case(control, dim)
    return U, starts, actions, geo, grid, pot, M.build_set(control, dim, DT, U, starts, actions)


def make_env(engine, control, dim, v_max=2.0, potential=False, grad_w=0.0):
    U, starts, actions, (md, org, res), grid, pot, _ = world(control, dim)
    env = engine.EnvMap(dim)
    env.setMap(org, md, grid, res)
    env.set_control(control)
    env.set_dt(DT)
    env.set_u(U)
    env.set_v_max(v_max)
    env.set_potential_weight(M.POT_W)
    env.set_gradient_weight(grad_w)
    if potential:
        env.set_potential_map(pot)
    return env


def model_samples(trajs, form, N=None, times=None):
    """[rows][K][count]; the rows of a trajectory without segments are SENTINEL (the call leaves them alone)."""
    rows = 4 * trajs[0].dim + (3 if form == M.COMMAND else 1)
    count = N + 1 if N is not None else np.asarray(times).shape[-1]
    out = np.full((rows, len(trajs), count), SENTINEL)
    for k, tr in enumerate(trajs):
        if tr.S == 0:
            continue
        out[:, k, :] = tr.sample(N, form) if N is not None else tr.evaluate(times if np.ndim(times) == 1 else times[k], form)
    return out


def shared_times():
    taus = [0.0]
    for _ in range(H):
        taus.append(DT + taus[-1])
    return np.array([-0.4, -1e-310, 0.0] + taus[1:] + [taus[-1] + 1e-9, 7.5, 1e12, 0.35, 1.05, 3.1415, np.nan, np.inf, -np.inf])


def own_times(trajs, Q=13):
    rng = np.random.default_rng(5)
    out = np.zeros((len(trajs), Q))
    for k, tr in enumerate(trajs):
        q = [-0.25, 0.0, tr.T, tr.T + 0.5, np.nextafter(tr.T, 0.0)] + [float(x) for x in tr.taus[1:-1]]
        q += [float(x) for x in rng.uniform(0, max(tr.T, 0.5), Q)]
        out[k] = q[:Q]
    return out


def upload(env, host):
    from motion_primitive_library_amd.env import DeviceArray
    host = np.ascontiguousarray(host)
    buf = DeviceArray(env, max(host.nbytes, 8))
    buf.upload(host)
    return buf


def padded_set(env, starts, actions, pad):
    """Device copies with strides `pad` entries larger than the counts."""
    F, n = starts.shape
    s = np.full((F, n + pad), np.nan)
    s[:, :n] = starts
    a = np.full((actions.shape[0], actions.shape[1] + pad), 10 ** 6, np.int32)
    a[:, :actions.shape[1]] = actions
    return upload(env, s), upload(env, a), n + pad, actions.shape[1] + pad


# ------------------------------------------------------------------------------------------- 1. info and samples
@pytest.mark.gpu
@pytest.mark.parametrize("control,dim", CASES, ids=IDS)
def test_info_and_samples_equal_the_model(engine, control, dim):
    U, starts, actions, geo, grid, pot, trajs = world(control, dim)
    F = 4 * dim + 2
    env = make_env(engine, control, dim)
    S = np.array([t.S for t in trajs], np.int32)
    assert sorted(set(S.tolist())) == [0, 1, 2, 3, 4, 5]

    # ---- info: host pointers
    info = env.traj_info(starts, actions, want_states=True)
    assert np.array_equal(info["n_segs"], S)
    assert np.array_equal(info["status"], np.array([t.status for t in trajs], np.uint8))
    same_bits(info["total_time"], np.array([t.T for t in trajs]), "total_time")
    same_bits(info["effort"], np.stack([t.effort for t in trajs], axis=1), "effort")
    want_states = np.zeros((F, H + 1, K))
    for k, t in enumerate(trajs):
        want_states[:, :t.S + 1, k] = np.stack(t.states).T
    same_bits(info["seg_state"], want_states, "seg_state")

    # ---- samples: host pointers, both forms, uniform and caller times, strides larger than the counts
    ts, to = shared_times(), own_times(trajs)
    for form in (M.COMMAND, M.WAYPOINT):
        rows = 4 * dim + (3 if form == M.COMMAND else 1)
        for what, kw, want in (("uniform", {"N": N_UNIFORM}, model_samples(trajs, form, N=N_UNIFORM)),
                               ("shared times", {"times": ts}, model_samples(trajs, form, times=ts)),
                               ("own times", {"times": to}, model_samples(trajs, form, times=to))):
            count = want.shape[2]
            out = np.full((4 * dim + 3, K + 3, count + 5), SENTINEL)
            got = env.traj_sample(starts, actions, form=form, out=out, **kw)
            assert got["samples"] is out
            same_bits(out[:rows, :K, :count], want, "%s form %d" % (what, form))
            untouched = np.ones(out.shape, bool)
            untouched[:rows, :K, :count] = False
            assert (out[untouched] == SENTINEL).all(), "%s form %d wrote outside its entries" % (what, form)
            assert np.array_equal(got["status"], info["status"])
    assert np.isnan(model_samples(trajs, M.COMMAND, times=ts)[:, S > 0, -3:]).all()  # the non-finite times

    # ---- one start state for all
    one = M.build_set(control, dim, DT, U, starts[:, 7:8], actions)
    got = env.traj_sample(starts[:, 7], actions, N=N_UNIFORM, out=np.full((4 * dim + 3, K, N_UNIFORM + 1), SENTINEL))
    same_bits(got["samples"], model_samples(one, M.COMMAND, N=N_UNIFORM), "n_starts = 1")
    same_bits(env.traj_info(starts[:, 7], actions)["effort"], np.stack([t.effort for t in one], axis=1), "n_starts = 1 effort")

    # ---- resident calls == host calls, padded strides, sentinels
    d_s, d_a, sstride, astride = padded_set(env, starts, actions, 11)
    dinfo = env.alloc_traj_info(K, H, want_states=True)
    dinfo.seg_state.upload(np.zeros((F, H + 1, K)))
    env.traj_info_resident(d_s, d_a, dinfo, H, n_starts=K, start_stride=sstride, action_stride=astride)
    env.synchronize()
    got = dinfo.download()
    for key in ("status", "n_segs", "total_time", "effort", "seg_state"):
        same_bits(got[key].astype(np.float64), info[key].astype(np.float64), "resident info " + key)
    for form, kw, host_kw in ((M.COMMAND, {"N": N_UNIFORM}, {"N": N_UNIFORM}), (M.WAYPOINT, {"N": N_UNIFORM}, {"N": N_UNIFORM}),
                              (M.COMMAND, {"times": ts, "n_times": len(ts), "time_stride": 0}, {"times": ts}),
                              (M.WAYPOINT, {"times": to, "n_times": to.shape[1], "time_stride": to.shape[1] + 2}, {"times": to})):
        count = N_UNIFORM + 1 if "N" in kw else kw["n_times"]
        if "times" in kw:
            t_host = kw["times"]
            if t_host.ndim == 2:
                t_host = np.concatenate([t_host, np.full((K, 2), np.nan)], axis=1)
            kw = dict(kw, times=upload(env, t_host))
        ds = env.alloc_traj_samples(K, count, n_stride=K + 2, sample_stride=count + 3)
        ds.out.upload(np.full((ds.rows, K + 2, count + 3), SENTINEL))
        env.traj_sample_resident(d_s, d_a, ds, H, form=form, n_starts=K, start_stride=sstride, action_stride=astride, **kw)
        env.synchronize()
        dev = ds.download()["samples"]
        host = env.traj_sample(starts, actions, form=form, out=np.full((ds.rows, K + 2, count + 3), SENTINEL), **host_kw)["samples"]
        same_bits(dev, host, "resident samples form %d %s" % (form, sorted(host_kw)))
        ds.free()
    for b in (d_s, d_a, dinfo):
        b.free()
    env.close()


# ------------------------------------------------------------------------------------------------- 2. traverse
@pytest.mark.gpu
@pytest.mark.parametrize("control,dim", CASES, ids=IDS)
def test_traverse_equals_the_model_under_every_lanes_value(engine, control, dim):
    U, starts, actions, (md, org, res), grid, pot, trajs = world(control, dim)
    seen_n = set()
    ended = {"free": 0, "sum": 0, "inf": 0}
    for name, with_pot, grad_w in M.MODES:
        env = make_env(engine, control, dim, potential=with_pot, grad_w=grad_w)
        d_s, d_a, sstride, astride = padded_set(env, starts, actions, 5)
        out = env.alloc_traj_traverse(K)
        for v_max in V_MAXES:
            env.set_v_max(v_max)
            want = M.traverse_set(trajs, grid, pot if with_pot else None, md, org, res, v_max, M.POT_W, grad_w)
            seen_n |= set(want["n_samples"].tolist())
            live = want["n_samples"] > 0
            ended["free"] += int((want["cost"][live] == 0).sum())
            ended["sum"] += int((np.isfinite(want["cost"][live]) & (want["cost"][live] > 0)).sum())
            ended["inf"] += int(np.isinf(want["cost"][live]).sum())
            for lanes in LANES:
                what = "%s v_max %g lanes %d" % (name, v_max, lanes)
                env.traj_traverse_resident(d_s, d_a, out, H, lanes=lanes, n_starts=K, start_stride=sstride, action_stride=astride)
                env.synchronize()
                got = out.download()
                same_bits(got["cost"], want["cost"], what + " cost")
                for key in ("status", "n_samples", "n_cells", "stop_sample"):
                    bad = np.nonzero(got[key] != want[key])[0]
                    assert bad.size == 0, "%s: %s differs for %s: got %s want %s" % (what, key, bad[:5], got[key][bad[:5]], want[key][bad[:5]])
            host = env.traj_traverse(starts, actions)
            same_bits(host["cost"], want["cost"], name + " host pointers cost")
            assert all(np.array_equal(host[k], want[k]) for k in ("status", "n_samples", "n_cells", "stop_sample"))
        for b in (d_s, d_a, out):
            b.free()
        env.close()
    assert min(seen_n - {0}) == 2 and max(seen_n) >= 290, sorted(seen_n)
    assert all(v >= 20 for v in ended.values()), ended


@pytest.mark.gpu
def test_alias_case_and_bad_trajectories(engine):
    md, org, res, U, start, actions, dt, v_max = M.alias_case()
    env = engine.EnvMap(2)
    env.setMap(org, md, np.zeros(64, np.int8), res)
    env.set_control(engine.VEL)
    env.set_dt(dt)
    env.set_u(U)
    env.set_v_max(v_max)
    for lanes in LANES:
        r = env.traj_traverse(start, actions, lanes=lanes)
        assert (r["cost"][0], r["n_samples"][0], r["n_cells"][0], r["stop_sample"][0], r["status"][0]) == (0.0, 2, 1, -1, 0), lanes
    # the same end point from a start one cell to the right: index 25 then 24 -- not skipped, outside, +inf
    start2 = start.copy()
    start2[0] = 1.5
    U2 = np.array([[7.0, -1.0]])
    env.set_u(U2)
    r = env.traj_traverse(start2, actions)
    assert np.isinf(r["cost"][0]) and r["stop_sample"][0] == 1 and r["n_cells"][0] == 2
    # bad actions: the segments before them; v_max * T / res >= 2^31: MPLX_TRAJ_BAD
    acts = np.array([[0, 0, -2, 0], [0, 1, 0, -1], [0, 0, 0, 0]], np.int32)
    info = env.traj_info(start2, acts)
    assert info["n_segs"].tolist() == [3, 1, 0, 1]
    assert info["status"].tolist() == [0, M.BAD_ACTION, M.BAD_ACTION | M.EMPTY, 0]
    env.set_v_max(4e9)
    r = env.traj_traverse(start2, acts)
    assert r["status"].tolist() == [M.BAD, M.BAD | M.BAD_ACTION, M.BAD_ACTION | M.EMPTY, M.BAD]
    assert np.isnan(r["cost"][[0, 1, 3]]).all() and r["cost"][2] == 0.0 and not r["n_samples"].any() and (r["stop_sample"] == -1).all()
    env.close()


@pytest.mark.gpu
def test_map_edit_between_two_traverse_calls(engine):
    md, org, res = [64, 48], [-1.0, 0.5], 0.25
    env = engine.EnvMap(2)
    env.setMap(org, md, np.zeros(64 * 48, np.int8), res)
    env.set_control(engine.VEL)
    env.set_dt(1.0)
    U = np.array([[1.0, 0.0], [1.0, 0.5]])
    env.set_u(U)
    env.set_v_max(2.0)
    start = np.zeros(10)
    start[:2] = [0.1, 3.1]
    actions = np.array([[0], [1], [0], [1]], np.int32)
    tr = M.Traj(engine.VEL, 2, 1.0, U, start, actions[:, 0])
    free = np.zeros(64 * 48, np.int8)
    want = M.traverse(tr, free, None, md, org, res, 2.0, 0.1, 0.0)
    got = env.traj_traverse(start, actions)
    assert got["cost"][0] == 0.0 == want["cost"] and got["stop_sample"][0] == -1 and got["n_cells"][0] == want["n_cells"]
    rows = tr.sample(want["n_samples"] - 1)
    idx, outside = M.cell_index(rows[:2], md, org, res)
    hit = int(idx[19])
    assert not outside.any() and hit != idx[0]
    env.editMap([hit], [100])
    free[hit] = 100
    want = M.traverse(tr, free, None, md, org, res, 2.0, 0.1, 0.0)
    got = env.traj_traverse(start, actions)
    assert np.isinf(got["cost"][0]) and got["stop_sample"][0] == want["stop_sample"] == int(np.nonzero(idx == hit)[0][0])
    assert got["n_cells"][0] == want["n_cells"]
    env.editMap([hit], [0])
    assert env.traj_traverse(start, actions)["cost"][0] == 0.0
    env.close()


# ------------------------------------------------------------------------------- 3. the planner's trajectory
@pytest.mark.gpu
def test_planner_trajectory_on_the_corridor_plan(engine):
    from test_plan_known_answer import corridor
    m = engine
    c = corridor()
    U = m.workloads.grid_controls([-0.5, 0.0, 0.5], 2)
    planner = m.MapPlanner(2, device=0)
    mu = m.MapUtil(2)
    mu.setMap(c["origin"], c["dim"], c["cells"].copy(), c["res"])
    planner.setMapUtil(mu)
    planner.setVmax(1.0)
    planner.setAmax(1.0)
    planner.setDt(1.0)
    planner.setU(U)
    assert planner.plan(m.Waypoint(2, m.ACC, pos=c["start"]), m.Waypoint(2, m.ACC, pos=c["goal"]))
    traj = planner.getTraj()
    assert traj.getTotalTime() == 35.0 and len(traj.actions) == 35
    info = planner.env.traj_info(traj.nodes[0], np.asarray(traj.actions).reshape(-1, 1))
    assert info["effort"][:, 0].tolist() == [36.75, 1.5, 0.0, 0.0, 0.0] and info["total_time"][0] == 35.0
    assert info["effort"][:4, 0].tolist() == [traj.J(k) for k in (m.VEL, m.ACC, m.JRK, m.SNP)]  # the planner's own summary
    assert traj.Jyaw() == 0.0 and traj.getSegmentTimes() == [1.0] * 35
    tr = M.Traj(m.ACC, 2, 1.0, U, traj.nodes[0], traj.actions)
    same_bits(traj.sample(35).T, tr.sample(35), "Trajectory.sample")
    assert np.array_equal(traj.sample(35)[:, :2], traj.getWaypoints()[:, :2])
    same_bits(traj.evaluate(17.0), tr.evaluate([17.0], M.COMMAND)[:, 0], "evaluate -> Command")
    same_bits(traj.evaluate(17.0, command=False), tr.evaluate([17.0], M.WAYPOINT)[:, 0], "evaluate -> Waypoint")
    assert planner.traverseTraj() == (0.0, -1) and planner.checkTraj()[0] == m.SLOT_FINITE
    # a cell of the path becomes occupied on the device: the stored trajectory no longer traverses
    rows = tr.sample(700)
    idx, _ = M.cell_index(rows[:2], c["dim"], c["origin"], c["res"])
    planner.env.editMap([int(idx[400])], [100])
    cost, stop = planner.traverseTraj()
    assert np.isinf(cost) and stop == int(np.nonzero(idx == idx[400])[0][0])
    planner.close()


# ------------------------------------------------------------------ 4. torch tensors, errors, nothing else moved
@pytest.mark.gpu
def test_torch_tensors_are_read_in_place(engine):
    control, dim = M.CONTROLS[6], 3
    U, starts, actions, geo, grid, pot, trajs = world(control, dim)
    env = make_env(engine, control, dim)
    t_s = torch.from_numpy(starts).to("cuda:0")
    t_a = torch.from_numpy(actions).to("cuda:0")
    t_out = torch.full((4 * dim + 3, K, N_UNIFORM + 1), SENTINEL, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()

    class View:  # a torch tensor as the sample rows
        n, rows = K, 4 * dim + 3

        def c_struct(self):
            s = engine._abi.TrajSampleOut()
            s.out, s.row_stride, s.sample_stride = t_out.data_ptr(), K * (N_UNIFORM + 1), N_UNIFORM + 1
            return s

    env.traj_sample_resident(t_s, t_a, View(), H, N=N_UNIFORM)
    out = env.alloc_traj_traverse(K)
    env.traj_traverse_resident(t_s, t_a, out, H)
    env.synchronize()
    same_bits(t_out.cpu().numpy(), model_samples(trajs, M.COMMAND, N=N_UNIFORM), "torch tensors")
    md, org, res = geo
    same_bits(out.download()["cost"], M.traverse_set(trajs, grid, None, md, org, res, 2.0, M.POT_W, 0.0)["cost"], "torch traverse")
    out.free()
    env.close()


@pytest.mark.gpu
def test_argument_and_state_errors(engine):
    A = engine._abi
    L = A.lib()
    control, dim = engine.ACC, 2
    U, starts, actions, (md, org, res), grid, pot, trajs = world(control, dim)
    starts = np.ascontiguousarray(starts)
    actions = np.ascontiguousarray(actions)

    env = engine.EnvMap(dim)
    ctx = env._ctx
    buf = np.zeros((4 * dim + 3, K, 8))
    cost = np.zeros(K)
    # the _device forms get device memory in every call that may launch: a kernel must never see a host address
    d_starts, d_actions, d_buf, d_cost = upload(env, starts), upload(env, actions), upload(env, buf), upload(env, cost)

    def make_set(dev, kw):
        s = A.TrajSet()
        s.starts, s.n_starts, s.start_stride = (d_starts.ptr if dev else starts.ctypes.data), K, K
        s.actions, s.n_traj, s.horizon, s.action_stride = (d_actions.ptr if dev else actions.ctypes.data), K, H, K
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def sample_out(dev, kw):
        o = A.TrajSampleOut()
        o.out, o.row_stride, o.sample_stride = (d_buf.ptr if dev else buf.ctypes.data), K * 8, 8
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def times(dev, kw):
        t = A.TrajTimes()
        t.form, t.n_uniform = A.TRAJ_COMMAND, 7
        for k, v in kw.items():
            setattr(t, k, (d_buf.ptr if dev else buf.ctypes.data) if v == "buffer" else v)
        return t

    def calls(set_kw={}, t_kw={}, so_kw={}, lanes=0, info_kw={}):
        """The three host-pointer calls, then the three _device calls, with the same overrides."""
        got = []
        for dev, sfx in ((False, ""), (True, "_device")):
            s, t, so = make_set(dev, set_kw), times(dev, t_kw), sample_out(dev, so_kw)
            io, to = A.TrajInfoOut(), A.TrajTraverseOut()
            to.cost = d_cost.ptr if dev else cost.ctypes.data
            for k, v in info_kw.items():
                setattr(io, k, v)
            got += [getattr(L, "mplx_traj_info" + sfx)(ctx, C.byref(s), C.byref(io)),
                    getattr(L, "mplx_traj_sample" + sfx)(ctx, C.byref(s), C.byref(t), C.byref(so)),
                    getattr(L, "mplx_traj_traverse" + sfx)(ctx, C.byref(s), lanes, C.byref(to))]
        return got

    none = {"n_traj": 0, "n_starts": 0, "start_stride": 0, "action_stride": 0}
    # ---- state errors, on a context that gets its state piece by piece (the C ABI directly: EnvMap sets params itself)
    assert calls() == [A.ERR_STATE] * 6                                     # no params
    env._flush()
    assert calls() == [A.ERR_STATE] * 6                                     # no controls
    env.set_control(control)
    env.set_dt(DT)
    env.set_u(U)
    env.set_v_max(2.0)
    env._flush()
    assert calls(none) == [A.OK, A.OK, A.ERR_STATE] * 2                     # no map: only traverse minds; n_traj = 0 is a no-op
    assert calls()[0::3] == [A.OK] * 2 and calls()[1::3] == [A.OK] * 2      # info and samples need no map
    env.setMap(org, md, grid, res)
    assert calls(none) == [A.OK] * 6
    env.set_v_max(-1.0)
    env._flush()
    assert calls()[2::3] == [A.ERR_STATE] * 2                               # traverse: v_max <= 0
    env.set_v_max(2.0)
    env._flush()
    env.set_control(engine.ACCxYAW)                                         # the table has no yaw column
    env._flush()
    assert calls() == [A.ERR_STATE] * 6
    env.set_control(control)
    env._flush()
    assert calls() == [A.OK] * 6

    # ---- argument errors
    for what, kw in (("horizon < 1", {"horizon": 0}), ("n_starts", {"n_starts": 2}), ("n_traj < 0", {"n_traj": -1}),
                     ("start_stride", {"start_stride": K - 1}), ("action_stride", {"action_stride": K - 1}),
                     ("NULL starts", {"starts": None}), ("NULL actions", {"actions": None})):
        assert calls(kw) == [A.ERR_ARG] * 6, what
    for what, kw in (("N < 0", {"n_uniform": -1}), ("form", {"form": 2}), ("Q < 1", {"n_uniform": 0, "n_times": 0}),
                     ("NULL times", {"n_uniform": 0, "n_times": 4}),
                     ("time_stride < Q", {"n_uniform": 0, "n_times": 4, "time_stride": 3, "times": "buffer"})):
        assert calls(t_kw=kw)[1::3] == [A.ERR_ARG] * 2, what
    for what, kw in (("sample_stride", {"sample_stride": 7}), ("row_stride", {"row_stride": K * 8 - 1})):
        assert calls(so_kw=kw)[1::3] == [A.ERR_ARG] * 2, what
    for lanes in (1, 8, 32, 128, -4):
        assert calls(lanes=lanes)[2::3] == [A.ERR_ARG] * 2, lanes
    assert calls(info_kw={"effort": d_buf.ptr, "effort_stride": K - 1})[0::3] == [A.ERR_ARG] * 2
    s, io = make_set(False, {}), A.TrajInfoOut()
    assert L.mplx_traj_info(ctx, None, C.byref(io)) == A.ERR_ARG and L.mplx_traj_info(ctx, C.byref(s), None) == A.ERR_ARG
    assert L.mplx_traj_sample(ctx, C.byref(s), None, C.byref(sample_out(False, {}))) == A.ERR_ARG
    assert L.mplx_traj_traverse(ctx, C.byref(s), 0, None) == A.ERR_ARG
    # every output pointer is optional
    assert calls(so_kw={"out": None}) == [A.OK] * 6
    # and the context still works after all of it
    want = M.traverse_set(trajs, grid, None, md, org, res, 2.0, M.POT_W, 0.0)
    same_bits(env.traj_traverse(starts, actions)["cost"], want["cost"], "after the error calls")
    for b in (d_starts, d_actions, d_buf, d_cost):
        b.free()
    env.close()


@pytest.mark.gpu
def test_expansion_before_and_after_trajectory_calls(engine):
    """The calls change nothing else in the context: one expansion before and after a series of them gives identical
    lists (blocked bits, free-box table and yaw pins stay valid)."""
    control, dim = engine.ACCxYAW, 2
    U, starts, actions, (md, org, res), grid, pot, trajs = world(control, dim)
    env = make_env(engine, control, dim, potential=True, grad_w=0.25)
    env.set_yaw_max(0.9)
    nodes = np.ascontiguousarray(starts[:, :64])
    before = env.expand_lists(nodes)
    for _ in range(2):
        env.traj_info(starts, actions, want_states=True)
        env.traj_sample(starts, actions, N=N_UNIFORM)
        env.traj_sample(starts, actions, times=shared_times(), form=M.WAYPOINT)
        for lanes in LANES:
            env.traj_traverse(starts, actions, lanes=lanes)
    after = env.expand_lists(nodes)
    assert sorted(before) == sorted(after)
    for key in before:
        assert np.array_equal(before[key], after[key], equal_nan=True), key
    env.close()
