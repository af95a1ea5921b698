"""GPU: mplx_heur_eval / mplx_heur_eval_device (include/mplx_heur.h) against tests/heur_model.py, bit for bit: every
supported (control, goal control) pair in 2-D and 3-D, a yaw control, pairs that keep the default, v_max <= 0, a NaN row,
the goal's own lattice state, sizes at the block edges, and the errors."""
import numpy as np
import pytest

import heur_model as HM

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4097]
# (control of the states, goal control; 0 = the states')
PAIRS = [("VEL", 0), ("ACC", 0), ("ACC", "VEL"), ("JRK", 0), ("JRK", "ACC"), ("JRK", "VEL"), ("ACCxYAW", 0), ("ACCxYAW", "ACC"),
         ("SNP", 0), ("VEL", "ACC")]
ORDER = {"VEL": HM.VEL, "ACC": HM.ACC, "JRK": HM.JRK, "SNP": HM.SNP}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def code(m, fn):
    with pytest.raises(m._abi.MplxError) as e:
        fn()
    return e.value.code


def same(got, want):
    """Bit for bit; any NaN equals any NaN (the payload of a NaN is not part of the interface)."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def make_env(m, D, control, w, v_max):
    env = m.EnvMap(D)
    env.set_control(getattr(m, control))
    env.set_w(w)
    env.set_v_max(v_max)
    env.set_dt(1.0)
    return env


def case_states(D, control, goal_control, K, seed):
    """K lattice columns with live rows up to the control's order (and a yaw), a goal with live velocity / acceleration;
    among them: the goal's own lattice state (column 0, and a copy a hair off it), dp = 0 with a live velocity, a NaN row."""
    rng = np.random.default_rng(seed)
    base = ORDER[control.replace("xYAW", "")]
    s = HM.lattice_states(rng, K, D, min(base, HM.JRK), zero_dp=0.05)
    F = 4 * D + 2
    if base == HM.SNP:
        s[3 * D:4 * D] = rng.integers(-4, 5, (D, K)) / 4.0
    if control.endswith("YAW"):
        s[4 * D] = rng.integers(-6, 7, K) * 0.1
    goal = np.zeros(F)
    goal[:D] = [0.5, -0.25, 0.75][:D]
    gbase = ORDER[goal_control] if goal_control else base
    if gbase >= HM.ACC:
        goal[D:2 * D] = [0.5, -0.25, 0.25][:D]
    if gbase >= HM.JRK:
        goal[2 * D:3 * D] = [-0.25, 0.5, 0.0][:D]
    s[:4 * D + 1, 0] = goal[:4 * D + 1]
    if K > 2:
        s[:, 1] = s[:, 0]
        s[0, 1] += 0.004  # rounds to the same lattice cell: h = 0 although the state differs
        s[:D, 2] = goal[:D]  # dp = 0
    if K > 3:
        s[D, 3] = np.nan
    if K > 4:
        s[0, 4] = np.inf
    return s, goal


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("control,goal_control", PAIRS, ids=["%s-%s" % (a, b or "same") for a, b in PAIRS])
def test_heur_eval_equals_the_model(engine, D, control, goal_control):
    m = engine
    gc = getattr(m, goal_control) if goal_control else 0
    ctl = getattr(m, control)
    for w, v_max in ((1.0, 2.0), (10.0, 3.0), (0.5, 0.0), (2.0, -1.0)):
        env = make_env(m, D, control, w, v_max)
        for K in (SIZES if w == 1.0 else [65]):
            s, goal = case_states(D, control, goal_control, K, 100 * D + K)
            want = HM.heur_eval(s, goal, ctl, gc, w, v_max, D, HM.ROBUST)
            got = env.heur_eval(s, goal, mode="robust", goal_control=gc)
            assert same(got, want), (control, goal_control, D, K, w, v_max)
            dflt = HM.heur_eval(s, goal, ctl, gc, w, v_max, D, HM.DEFAULT)
            assert same(env.heur_eval(s, goal, mode="default", goal_control=gc), dflt), (control, goal_control, D, K)
            ok = ~np.isnan(want)
            assert np.all(want[ok] >= dflt[ok])  # never below the default
            if K >= 65:
                assert np.isnan(want[3]) and np.isnan(want[4])
                if not goal_control:  # (a goal under another flag hashes other rows: no state is "the goal's own")
                    assert want[0] == 0.0 and want[1] == 0.0
                if ORDER[control.replace("xYAW", "")] <= HM.JRK and (not goal_control or ORDER[goal_control] <= ORDER[control.replace("xYAW", "")]):
                    assert np.sum(want[ok] > dflt[ok]) > K // 2  # the dynamics say something on most columns
                else:
                    assert same(want[5:], dflt[5:])  # SNP, and a goal with more derivatives than the state: the default
        env.close()


@pytest.mark.parametrize("D", [2, 3])
def test_heur_eval_resident_equals_the_model(engine, D):
    """Resident rows with a stride above n: a frontier's layout; the entries of `out` behind n stay as they were."""
    m = engine
    w, v_max = 1.0, 2.0
    env = make_env(m, D, "JRK", w, v_max)
    for K in SIZES:
        s, goal = case_states(D, "JRK", "ACC", K, 7 * K + D)
        fr = m.TableFrontier(env, K, spare=3)
        st = np.zeros((env.n_fields, fr.state_stride))
        st[:, :K] = s
        st[:, K:] = np.nan
        fr.state.upload(st)
        out = m.DeviceArray(env, (K + 3) * 8)
        out.upload(np.full(K + 3, -7.0))
        env.heur_eval_resident(fr, goal, out, goal_control=m.ACC)
        env.synchronize()
        got = out.download(np.float64, (K + 3,))
        want = HM.heur_eval(s, goal, m.JRK, m.ACC, w, v_max, D, HM.ROBUST)
        assert same(got[:K], want), (D, K)
        assert np.all(got[K:] == -7.0)
        out.free()
        fr.free()
    env.close()


def test_heur_eval_errors(engine):
    m = engine
    A = m._abi
    L = A.lib()
    env = make_env(m, 2, "ACC", 1.0, 2.0)
    s, goal = case_states(2, "ACC", 0, 8, 1)
    assert code(m, lambda: env.heur_eval(s, goal, mode="reference")) == A.ERR_ARG   # host only
    assert code(m, lambda: env.heur_eval(s, goal, mode=7)) == A.ERR_ARG
    assert code(m, lambda: env.heur_eval(s, goal, mode="robust", w=0.0)) == A.ERR_ARG
    assert code(m, lambda: env.heur_eval(s, goal, mode="robust", w=-1.0)) == A.ERR_ARG
    assert code(m, lambda: env.heur_eval(s, goal, mode="robust", w=float("nan"))) == A.ERR_ARG
    assert code(m, lambda: env.heur_eval(s, goal, mode="robust", goal_control=5)) == A.ERR_ARG
    env.heur_eval(s, goal, mode="default", w=0.0)  # the default takes any w, as it always did
    out = m.DeviceArray(env, 64)
    dev = m.DeviceArray(env, s.nbytes)
    dev.upload(s)
    assert code(m, lambda: env.heur_eval_resident(dev, goal, out, n=8, stride=8, mode="reference")) == A.ERR_ARG
    assert code(m, lambda: env.heur_eval_resident(dev, goal, out, n=8, stride=7)) == A.ERR_ARG
    assert code(m, lambda: env.heur_eval_resident(dev, goal, out, n=-1, stride=8)) == A.ERR_ARG
    g, keep = env._heur_goal(goal, 0, None, None)
    import ctypes as C
    assert L.mplx_heur_eval(None, C.byref(g), 2, None, 0, 0, None) == A.ERR_ARG
    assert L.mplx_heur_eval(env._ctx, None, 2, None, 0, 0, None) == A.ERR_ARG
    assert L.mplx_heur_eval(env._ctx, C.byref(g), 2, None, 0, 0, None) == A.OK       # K == 0: a no-op
    assert L.mplx_heur_eval(env._ctx, C.byref(g), 2, None, 4, 4, None) == A.ERR_ARG
    env.heur_eval_resident(dev, goal, out, n=8, stride=8)
    env.synchronize()
    assert same(out.download(np.float64, (8,)), HM.heur_eval(s, goal, m.ACC, 0, 1.0, 2.0, 2, HM.ROBUST))
    out.free()
    dev.free()
    env.close()
