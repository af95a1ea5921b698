"""What the staging walks share (tests/test_gpu_staging.py, test_gpu_staging_sets.py, test_gpu_staging_search.py): the
order of a walk as data, the world of a configuration, poisoned rows and the byte-for-byte comparison."""
import ctypes as C

import numpy as np

from motion_primitive_library_amd import workloads as W

POISON = 0xA5
SIZES = (1, 3, 65, 257, 1000)
CONFIGS = {"2d_acc_yaw": (2, W.ACCxYAW, (48, 40)), "3d_acc": (3, W.ACC, (20, 18, 16))}


def schedule(kinds, seed):
    """[(kind, n, visit)]: a closed walk over every ordered pair of `kinds`, every step of it at the largest size; the first
    four visits of a kind are preceded by the same kind at one of the four smaller sizes.  visit counts the earlier steps
    of the same kind (the variant of a call is picked by it)."""
    k = len(kinds)
    rng = np.random.default_rng(seed)
    out = {a: [int(b) for b in rng.permutation([b for b in range(k) if b != a])] for a in range(k)}
    stack, walk = [0], []
    while stack:  # Hierholzer: a closed walk over every arc of the complete digraph
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            walk.append(stack.pop())
    steps, visits = [], [0] * k
    for v in reversed(walk):
        if visits[v] < len(SIZES) - 1:
            steps.append((kinds[v], SIZES[(visits[v] + v) % (len(SIZES) - 1)], 2 * visits[v]))
        steps.append((kinds[v], SIZES[-1], 2 * visits[v] + 1 if visits[v] < len(SIZES) - 1 else visits[v] + len(SIZES) - 1))
        visits[v] += 1
    return steps


class World:
    """The map, controls, limits and goal of a configuration (numpy only; the same for every context of a walk)."""

    def __init__(self, name):
        self.dim, self.control, self.map_dim = CONFIGS[name]
        self.res, self.origin = 0.1, [0.0] * self.dim
        self.cells = W.box_map(self.map_dim, self.res, 0.15, 1017, side_m=(0.2, 0.8))  # [z][y][x]; editMap steps change it
        yaw = [-0.5, 0.0, 0.5] if self.control & 0x10 else None
        self.U = W.grid_controls([-1, 0, 1], self.dim, yaw_rates=yaw)
        self.params = {"v_max": 2.0, "yaw_max": 0.5} if yaw else {"v_max": 2.0}
        self.F, self.nU = 4 * self.dim + 2, self.U.shape[0]
        probe = W.random_frontier(self.cells, self.origin, self.res, 1, 7, self.control, 2.0, 0.5)
        self.goal = probe[:, 0].copy()

    def configure(self, env):
        env.setMap(self.origin, list(self.map_dim), self.cells, self.res)
        env.set_control(self.control)
        env.set_u(self.U)
        for k, v in self.params.items():
            getattr(env, "set_" + k)(v)
        env.set_goal(self.goal, tol_pos=1.0)
        env._flush()


def poisoned(dtype, shape):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = POISON
    return a


def fill(struct, ptrs, **extra):
    for k, p in ptrs.items():
        setattr(struct, k, p)
    for k, v in extra.items():
        setattr(struct, k, v)
    return struct


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def assert_same_bytes(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in got:
        assert np.array_equal(raw(got[k]), raw(want[k])), "%s: row `%s` differs in %d bytes" % (
            what, k, int((raw(got[k]) != raw(want[k])).sum()))


# ---- what the walks over long-lived objects add
def ptr(a):
    """The address of a host array (None: a row that is not asked for)."""
    return None if a is None else a.ctypes.data


class Device:
    """Device copies of the inputs and poisoned device rows of one twin call on `env`; freed together."""

    def __init__(self, engine, env):
        self.engine, self.env, self.bufs = engine, env, []

    def up(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        b = self.engine.DeviceArray(self.env, max(a.nbytes, 8))
        if a.nbytes:
            b.upload(a)
        self.bufs.append(b)
        return b.ptr

    def rows(self, spec):
        """name -> device address of a poisoned row per (dtype, shape) of `spec`; download() reads them all back."""
        abi = self.engine._abi
        self.spec, self.out = spec, {}
        for k, (dt, shape) in spec.items():
            b = self.engine.DeviceArray(self.env, max(int(np.prod(shape)) * np.dtype(dt).itemsize, 8))
            abi.check(self.env._ctx, abi.lib().mplx_memset(self.env._ctx, b.ptr, POISON, b.nbytes))
            self.bufs.append(b)
            self.out[k] = b
        return {k: b.ptr for k, b in self.out.items()}

    def download(self):
        self.env.synchronize()
        return {k: self.out[k].download(dt, shape) for k, (dt, shape) in self.spec.items()}

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def disturb(abi, env, n_cells):
    """Two host calls of another kind on the long-lived context, between a setter and the call that reads what it set:
    mplx_read_cells at n = 1000 overwrites the head of the arena (and frees the block where it grows it), at n = 1 it
    runs a tiny layout in a large block.  An object that kept a pointer into the arena then reads something else."""
    L = abi.lib()
    for n in (1000, 1):
        idx = (np.arange(n, dtype=np.int64) * 7919) % n_cells
        vals = poisoned("i1", (n,))
        abi.check(env._ctx, L.mplx_read_cells(env._ctx, 0, idx.ctypes.data, n, vals.ctypes.data))


def handle(abi, ctx, create, *args):
    h = C.c_void_p()
    abi.check(ctx, create(*args, C.byref(h)))
    return h
