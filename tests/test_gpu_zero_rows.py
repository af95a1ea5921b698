"""GPU: state rows a launch can only fill with +0.0 are not stored to when the caller vouches they hold it already
(mplx_lists_zero_fill / mplx_expand_lists_device_z / mplx_last_lists_zero_rows, include/mplx.h).

The promise is a mask beside the buffer, so every way it can go wrong is a stale row nothing else detects.  Checked here:
  1. every kernel of the GRID route (lex, general, pair) and the TILE / DENSE routes, 2D / 3D x VEL / ACC / JRK and
     ACCxYAW on a potential map: a launch with the mask into a zero-filled buffer against a launch through the old entry
     point into a buffer filled with 0xA5 -- every used entry of every row equal as bit patterns, both equal to the
     oracle, and the set of rows actually skipped equal to the set computed here from the control flag (so the test
     cannot pass because nothing was ever skipped);
  2. mask transitions on ONE buffer (ACC -> JRK -> ACC, ACC -> ACCxYAW -> ACC, VEL -> ACC -> VEL) with a shrinking
     frontier in the last step: a row an earlier launch dirtied is written again;
  3. a voided promise (rows overwritten, mask 0) and zero_rows == NULL: every row written;
  4. what a launch may not write stays what it was, line padding of skipped rows included (a control table large enough
     for the padding rule, kLinePadMinControls)."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_lists_equal, engine_env, oracle_env
from test_gpu_parity import _small_world

pytestmark = pytest.mark.gpu
YAW_COST_RTOL = 1e-6
POISON = 0xA5
POISON_U64 = np.frombuffer(bytes([POISON] * 8), dtype=np.uint64)[0]
VEL, ACC, JRK, ACCxYAW = 0x01, 0x03, 0x07, 0x13


def const_rows(dim, control):
    """Rows a control can only fill with +0.0: derivative rows of order above the control's (state row = order * dim +
    axis; VEL is order 1, ACC 2, JRK 3), and the yaw row (4 * dim) without the yaw bit -- restated from the reference's
    Primitive (primitive.h: a polynomial of degree K has zero derivatives above K; :322 yaw = 0), not from the engine."""
    order = {0x01: 1, 0x03: 2, 0x07: 3, 0x0F: 4}[control & 0x0F]
    m = 0
    for b in range(order + 1, 4):
        for i in range(dim):
            m |= 1 << (b * dim + i)
    if not control & 0x10:
        m |= 1 << (4 * dim)
    return m


def _full(dim):
    return (1 << (4 * dim + 2)) - 1


def _poison(env, lists, state_only=False, keep_state=False):
    """0xA5 into every byte of the rows (the mask of a Lists whose state rows are overwritten is void: 0)."""
    L, ck = env._abi_lib, env._abi_check
    n = max(lists.n_slots, 1)
    if not keep_state:
        ck(L.mplx_memset(env._ctx, lists.state.ptr, POISON, lists.state_stride * 8 * lists.n_fields))
        lists.zero_rows = 0
    if not state_only:
        for buf, isz in ((lists.action, 4), (lists.cost, 8), (lists.hash, 8), (lists.iters, 4)):
            if buf is not None:
                ck(L.mplx_memset(env._ctx, buf.ptr, POISON, n * isz))
        ck(L.mplx_memset(env._ctx, lists.count.ptr, POISON, max(lists.n_nodes, 1) * 4))


def _env(engine, wl, route="grid"):
    env = engine_env(engine, wl)
    abi = engine._abi
    env._abi_lib = abi.lib()
    env._abi_check = lambda rc: abi.check(env._ctx, rc)
    env.set_lists_route(route)
    return env


def _launch_old(engine, env, fr, lists, n=None):
    """mplx_expand_lists_device itself (EnvMap.expand_lists_resident would take the _z entry point for a Lists)."""
    env._flush()
    s = lists.c_struct()
    n = fr.n_nodes if n is None else int(n)
    env._abi_check(env._abi_lib.mplx_expand_lists_device(env._ctx, fr.ptr, n, fr.n_nodes, C.byref(s)))
    lists.zero_rows = 0


def _used(got, n=None):
    S = int(got["stride"])
    count = got["count"] if n is None else got["count"][:n]
    return (np.arange(S)[None, :] < count[:, None]).ravel()


def _same_used(a, b, what, n=None):
    """Two engine list sets: identical counts and, over the used prefix of every node's list, every row bit for bit."""
    ca, cb = (a["count"], b["count"]) if n is None else (a["count"][:n], b["count"][:n])
    assert np.array_equal(ca, cb), what
    used = _used(a, n)
    m = used.size
    for k in ("action", "hash", "iters"):
        assert np.array_equal(a[k][:m][used], b[k][:m][used]), "%s: %s differs" % (what, k)
    assert np.array_equal(a["cost"][:m][used].view(np.uint64), b["cost"][:m][used].view(np.uint64)), "%s: cost differs" % what
    ga, gb = a["state"][:, :m][:, used].view(np.uint64), b["state"][:, :m][:, used].view(np.uint64)
    bad = np.argwhere(ga != gb)
    assert bad.shape[0] == 0, "%s: state differs in %d entries, first (row, entry) %s" % (what, bad.shape[0], bad[:3].tolist())
    return used


def _rows_all_zero(state, mask, what):
    """Every entry, used or not, of the rows in `mask` is +0.0 as a bit pattern."""
    u = state.view(np.uint64)
    for f in range(state.shape[0]):
        if (mask >> f) & 1:
            assert not u[f].any(), "%s: state row %d is in the mask and holds a non-zero bit pattern" % (what, f)


def _world(engine, dim, control, seed, n_nodes, potential=False):
    wl = _small_world(engine, dim, control, seed=seed, n_nodes=n_nodes, potential=potential)
    if control & 0x10:
        wl.U = engine.workloads.grid_controls([-1.0, 0.0, 1.0], dim, yaw_rates=[-0.5, 0.0, 0.5])
        wl.params["wyaw"] = 1.0
        wl.params["yaw_max"] = 0.9
    if potential:
        wl.params["gradient_weight"] = 0.0
    return wl


# (kernel or route, dim, control): the lex kernel, the general kernel on the same tables (MPLX_GRID_LEX=0), the pair kernel
# (yaw on a potential map over a pre-screened frontier), and the two routes that store every row
CASES = [(k, d, c) for k in ("lex", "grid") for d in (2, 3) for c in (VEL, ACC, JRK)] + \
        [("pair", 2, ACCxYAW), ("pair", 3, ACCxYAW), ("grid-yaw", 2, ACCxYAW), ("grid-yaw", 3, ACCxYAW)] + \
        [(r, d, c) for r in ("tile", "dense") for d, c in ((2, VEL), (3, ACC), (2, JRK))]


@pytest.mark.parametrize("kind,dim,control", CASES)
def test_masked_launch_equals_unmasked_launch_and_the_oracle(engine, oracle_lib, monkeypatch, kind, dim, control):
    if kind == "grid":
        monkeypatch.setenv("MPLX_GRID_LEX", "0")
    if kind == "pair":
        monkeypatch.setenv("MPLX_GRID_PRESCREEN_MIN", "1")
        monkeypatch.setenv("MPLX_GRID_PAIR", "1")
    wl = _world(engine, dim, control, seed=8100 + 10 * dim + control, n_nodes=333 if kind == "pair" else 200,
                potential=(kind == "pair"))
    wl.nodes[dim:4 * dim, ::10] = 0.0  # nodes at rest: the dropped successor shifts the list
    what = "%s dim%d ctrl0x%x" % (kind, dim, control)
    ref = oracle_lib.expand(oracle_env(wl), wl.nodes, threads=8)
    route = kind if kind in ("tile", "dense") else "grid"
    env = _env(engine, wl, route)
    fr = env.upload_frontier(wl.nodes)
    # with the mask, into a zero-filled buffer
    a = env.alloc_lists(wl.n_nodes, want_state=True, want_iters=True)
    assert a.zero_rows == _full(dim)
    env.expand_lists_resident(fr, a)
    env.synchronize()
    skipped, after = env.last_lists_zero_rows(), a.zero_rows
    assert env.last_lists_route() == route
    if route == "grid":
        assert env.last_grid_kernel() == {"grid-yaw": "grid"}.get(kind, kind), what
    want = const_rows(dim, control) if route == "grid" else 0
    print("%s: skipped 0x%x, mask after 0x%x, expected 0x%x" % (what, skipped, after, want))
    assert skipped == want, "%s: rows skipped 0x%x, expected 0x%x" % (what, skipped, want)
    assert after == want, "%s: mask after the launch 0x%x, expected 0x%x" % (what, after, want)
    got_a = a.download()
    # without, through the old entry point, into a buffer of 0xA5
    b = env.alloc_lists(wl.n_nodes, want_state=True, want_iters=True)
    _poison(env, b)
    _launch_old(engine, env, fr, b)
    env.synchronize()
    assert env.last_lists_zero_rows() == 0, what
    got_b = b.download()
    for lists in (a, b):
        lists.free()
    fr.free()
    env.close()
    used = _same_used(got_a, got_b, what)
    assert used.any()
    assert not (got_b["state"][:, used].view(np.uint64) == POISON_U64).any(), "%s: the old entry point left a used entry unwritten" % what
    rtol = YAW_COST_RTOL if control & 0x10 else 0.0
    assert_lists_equal(got_a, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=rtol, what=what + " (mask)")
    assert_lists_equal(got_b, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=rtol, what=what + " (old entry point)")
    _rows_all_zero(got_a["state"], after, what)


SEQUENCES = [("ACC-JRK-ACC", (ACC, JRK, ACC)), ("ACC-ACCxYAW-ACC", (ACC, ACCxYAW, ACC)), ("VEL-ACC-VEL", (VEL, ACC, VEL))]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name,controls", SEQUENCES)
def test_mask_transitions_on_one_buffer(engine, oracle_lib, dim, name, controls):
    """One buffer through three launches with different controls (a context per control: the mask belongs to the buffer,
    the library keeps no record), the last one over a shorter frontier.  After every step the used entries equal those
    of a fresh context writing into a buffer of 0xA5 through the old entry point, and the rows skipped are exactly the
    rows that are constant for this control AND have been constant for every control before it."""
    N = (240, 240, 90)
    wls = [_world(engine, dim, c, seed=8300 + 10 * dim + i, n_nodes=N[i]) for i, c in enumerate(controls)]
    stride = max((w.U.shape[0] + 31) & ~31 for w in wls)
    envs = [_env(engine, w) for w in wls]
    lists = envs[0].alloc_lists(max(N), want_state=True, want_iters=True, stride=stride)
    mask = _full(dim)
    assert lists.zero_rows == mask
    for step, (wl, env, control) in enumerate(zip(wls, envs, controls)):
        what = "%s dim%d step %d (0x%x)" % (name, dim, step, control)
        fr = env.upload_frontier(wl.nodes)
        env.expand_lists_resident(fr, lists, wl.n_nodes)
        env.synchronize()
        want = mask & const_rows(dim, control)
        print("%s: skipped 0x%x, expected 0x%x" % (what, env.last_lists_zero_rows(), want))
        assert env.last_lists_zero_rows() == want, what
        assert lists.zero_rows == want, what
        mask = want
        got = lists.download()
        # a fresh context and a fresh buffer of 0xA5, the old entry point
        fresh_env = _env(engine, wl)
        fresh = fresh_env.alloc_lists(max(N), want_state=True, want_iters=True, stride=stride)
        _poison(fresh_env, fresh)
        ffr = fresh_env.upload_frontier(wl.nodes)
        _launch_old(engine, fresh_env, ffr, fresh, wl.n_nodes)
        fresh_env.synchronize()
        want_lists = fresh.download()
        fresh.free()
        ffr.free()
        fresh_env.close()
        fr.free()
        used = _same_used(got, want_lists, what, n=wl.n_nodes)
        assert used.any()
        _rows_all_zero(got["state"], mask, what)
        ref = oracle_lib.expand(oracle_env(wl), wl.nodes, threads=8)
        for g in (got, want_lists):
            g["count"] = g["count"][:wl.n_nodes]
        assert_lists_equal(got, ref, wl.n_nodes, wl.U.shape[0], cost_rtol=YAW_COST_RTOL if control & 0x10 else 0.0, what=what)
    # the middle launch dirtied rows that are constant for the last control: they were written again, not skipped
    dirtied = const_rows(dim, controls[2]) & ~const_rows(dim, controls[1])
    assert dirtied and not (mask & dirtied), "%s: the sequence does not exercise a dirtied row" % name
    lists.free()
    for env in envs:
        env.close()


def test_a_voided_promise_and_a_null_mask_write_every_row(engine, oracle_lib):
    dim, control = 3, ACC
    wl = _world(engine, dim, control, seed=8500, n_nodes=150)
    ref = oracle_lib.expand(oracle_env(wl), wl.nodes, threads=8)
    env = _env(engine, wl)
    fr = env.upload_frontier(wl.nodes)
    # zero-filled, then overwritten: the caller passes 0
    a = env.alloc_lists(wl.n_nodes, want_state=True, want_iters=True)
    assert a.zero_rows == _full(dim)
    _poison(env, a, state_only=True)
    assert a.zero_rows == 0
    env.expand_lists_resident(fr, a)
    env.synchronize()
    assert env.last_lists_zero_rows() == 0 and a.zero_rows == 0
    got_a = a.download()
    used = _used(got_a)
    assert not (got_a["state"][:, used].view(np.uint64) == POISON_U64).any(), "a used entry still holds 0xA5"
    assert_lists_equal(got_a, ref, wl.n_nodes, wl.U.shape[0], what="voided promise")
    # zero_rows == NULL is the old entry point
    b = env.alloc_lists(wl.n_nodes, want_state=True, want_iters=True)
    _poison(env, b)
    s = b.c_struct()
    env._abi_check(env._abi_lib.mplx_expand_lists_device_z(env._ctx, fr.ptr, wl.n_nodes, fr.n_nodes, C.byref(s), None))
    env.synchronize()
    assert env.last_lists_zero_rows() == 0
    got_b = b.download()
    _same_used(got_a, got_b, "NULL mask vs mask 0")
    assert not (got_b["state"][:, used].view(np.uint64) == POISON_U64).any()
    # the state setter voids the mask (a fresh allocation is not zero)
    c = env.alloc_lists(8, want_state=True)
    assert c.zero_rows == _full(dim)
    old = c.state
    c.state = engine.DeviceArray(env, old.nbytes)
    assert c.zero_rows == 0
    old.free()
    # lists without state rows promise nothing
    d = env.alloc_lists(8, want_state=False)
    assert d.zero_rows == 0
    for lists in (a, b, c, d):
        lists.free()
    fr.free()
    env.close()


@pytest.mark.parametrize("dim,control,n_vals,kind", [(3, ACC, 7, "lex"), (2, VEL, 18, "lex"), (3, ACC, 7, "grid"), (2, JRK, 16, "lex")])
def test_entries_a_launch_may_not_write_stay_what_they_were(engine, oracle_lib, monkeypatch, dim, control, n_vals, kind):
    """A control table of >= 256 entries (the line-padding rule), more nodes allocated than launched, state rows
    zero-filled and every other row 0xA5: state entries outside (used + line padding) are still +0.0, the other rows'
    still 0xA5, and the skipped rows hold +0.0 in EVERY entry -- their padding lanes are skipped too -- while the padding
    of a row that is stored (t: never zero here) is written, i.e. the padding rule was in force."""
    if kind == "grid":
        monkeypatch.setenv("MPLX_GRID_LEX", "0")
    n, extra = 70, 9
    wl = _small_world(engine, dim, control, seed=8600 + n_vals + dim, n_nodes=n)
    wl.U = engine.workloads.grid_controls(list(np.linspace(-1.0, 1.0, n_vals)), dim)
    nU = wl.U.shape[0]
    assert nU >= 256
    wl.nodes[4 * dim + 1] += 1.0  # t > 0: the t row of every successor is non-zero
    # (VEL with 18 values per axis: 324 successors per node -- with an odd number of values the zero control is dropped
    # from every list and 17^2 - 1 = 288 entries end on a line, which leaves no padding to look at)
    what = "%s dim%d ctrl0x%x %d controls" % (kind, dim, control, nU)
    ref = oracle_lib.expand(oracle_env(wl), wl.nodes, threads=8)
    env = _env(engine, wl)
    full = np.concatenate([wl.nodes, np.zeros((wl.nodes.shape[0], extra))], axis=1)
    fr = env.upload_frontier(full)
    lists = env.alloc_lists(n + extra, want_state=True, want_iters=True)
    S = lists.stride
    assert S % 32 == 0
    _poison(env, lists, keep_state=True)
    assert lists.zero_rows == _full(dim)
    env.expand_lists_resident(fr, lists, n)
    env.synchronize()
    assert env.last_grid_kernel() == kind
    want = const_rows(dim, control)
    assert env.last_lists_zero_rows() == want and lists.zero_rows == want, what
    got = lists.download()
    lists.free()
    fr.free()
    env.close()
    cap = (n + extra) * S
    count = got["count"][:n]
    assert (got["count"][n:] == np.frombuffer(bytes([POISON] * 4), dtype=np.int32)[0]).all(), "%s: count written past n_nodes" % what
    j = np.arange(cap) % S
    cnt = np.zeros(cap, np.int64)
    cnt[:n * S] = np.repeat(count, S)
    used = (np.arange(cap) < n * S) & (j < cnt)
    pad16 = (np.arange(cap) < n * S) & ~used & (j < ((cnt + 15) & ~15))
    pad32 = (np.arange(cap) < n * S) & ~used & (j < ((cnt + 31) & ~31))
    st = got["state"].view(np.uint64)
    outside = ~(used | pad16)
    assert not st[:, outside].any(), "%s: a state entry outside the used and padding entries was written" % what
    for k, isz, pad in (("action", 4, pad32), ("iters", 4, pad32), ("cost", 8, pad16), ("hash", 8, pad16)):
        u = got[k].view("<u%d" % isz)
        poison = np.frombuffer(bytes([POISON] * isz), dtype=u.dtype)[0]
        assert (u[~(used | pad)] == poison).all(), "%s: row `%s` written outside what a launch may write" % (what, k)
    _rows_all_zero(got["state"], want, what)
    assert pad16.any() and st[4 * dim + 1][pad16].all(), "%s: the line padding of the t row was not written" % what
    got["count"] = count
    assert_lists_equal(got, ref, n, nU, what=what)
