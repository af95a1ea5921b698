"""Polynomial trajectory sets on the device (mplx_poly of include/mplx_solve.h): PolyTrajSet with its limits
(include/mplx_limits.h), time scaling (include/mplx_scale.h) and conflicts (include/mplx_conflict.h), and the helpers
that build the conflict input."""
import ctypes as C

import numpy as np

from . import _abi
from .rows import Conflicts, ConflictResult, LambdaRows, PolyLimits, TrajInfo, TrajTraverse, _device_ptr

TRAJ_COMMAND = _abi.TRAJ_COMMAND


class ShortcutResult:
    """What EnvMap.shortcut / SearchResult.shortcut return (mplx_shortcut, include/mplx_limits.h).  poly: the PolyTrajSet of
    the Q shortcut trajectories; pairs: the PolyTrajSet of the Q (w_max - 1) max_hop pair problems (pair (k, i, j) at
    (k (w_max - 1) + i) max_hop + (j - i - 1)); per query status (0, SOLVE_EMPTY, SHORTCUT_BAD_CHAIN), keep (a list of
    ascending state indices; keep_rows: the call's own [w_max][Q] rows, -1 past n_keep), cost, chain_cost; edge_cost
    [Q][w_max - 1][max_hop] (+inf: not admitted).  chain_hit: None, or after a timed shortcut (avoid=; include/
    mplx_reserve_poly.h) per query the smallest (instant << 32 | reservation) at which one of the chain's OWN edges meets the
    table as it is now, -2 if none does but one leaves the table's horizon, -1 if the chain still holds.  free() it."""

    def __init__(self, poly, pairs, max_hop, rows):
        self.poly, self.pairs, self.max_hop = poly, pairs, int(max_hop)
        self.status, self.n_keep, self.cost, self.chain_cost = rows["status"], rows["n_keep"], rows["cost"], rows["chain_cost"]
        self.keep_rows = rows["keep"]
        self.keep = [rows["keep"][:n, k].copy() for k, n in enumerate(self.n_keep)]
        self.edge_cost = rows["edge_cost"]
        self.chain_hit = rows.get("chain_hit")

    def segments(self, k):
        """The shortcut trajectory of query k on the host, as EnvMap.load_traj takes one: (coeff [S][D + 1][6], dts [S]),
        segment s the pair problem between the kept states keep[k][s] and keep[k][s + 1]."""
        keep, w1 = self.keep[k], self.poly.n_wmax - 1
        idx = [(k * w1 + int(i)) * self.max_hop + int(j - i - 1) for i, j in zip(keep[:-1], keep[1:])]
        return self.pairs.segments()[0][:, :, idx].transpose(2, 0, 1).copy(), self.pairs.dts()[0, idx].copy()

    def free(self):
        self.poly.free()
        self.pairs.free()


def _conflict_in(K, step, n_steps, t0, radius, group, rank, park, chunk_steps, device):
    """mplx_conflict_in from host arrays ([K] or a scalar to repeat) or, device=True, from device buffers; (struct, keep)."""
    i, keep = _abi.ConflictIn(), []
    i.step, i.n_steps, i.chunk_steps = float(step), int(n_steps), int(chunk_steps)
    i.mode = _abi.CONFLICT_PARK if park else _abi.CONFLICT_GONE
    if radius is None:
        raise ValueError("conflicts: give a radius (a scalar or [K])")

    def ptr(v, dtype):
        if device:
            return _device_ptr(v)
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (K,)))
        keep.append(a)
        return a.ctypes.data

    if t0 is not None:
        i.t0 = ptr(t0, np.float64)
    if np.ndim(radius) == 0 and not hasattr(radius, "ptr") and not hasattr(radius, "data_ptr"):
        i.radius_all = float(radius)
    else:
        i.radius = ptr(radius, np.float64)
    if group is not None:
        i.group = ptr(group, np.int32)
    if rank is not None:
        i.rank = ptr(rank, np.int32)
    return i, keep


def _conflict_steps(step, t0, total, ok):
    """The smallest n_steps whose instants i * step cover max(t0 + total) over the trajectories without a status."""
    if not (step > 0 and np.isfinite(step)):
        raise ValueError("conflicts: step must be > 0 and finite")
    K = len(total)
    t0 = np.zeros(K) if t0 is None else np.broadcast_to(np.asarray(t0, dtype=np.float64), (K,))
    end = np.where(np.asarray(ok, dtype=bool) & np.isfinite(t0), t0 + total, 0.0)
    last = max(float(end.max()) if K else 0.0, 0.0)
    return min(int(np.ceil(last / step)) + 1, 2 ** 31 - 1)


def _conflict_host_out(K, want_pairs):
    """The host twin of Conflicts, preset to `no conflict` (-1, -1, inf)."""
    rows, o = Conflicts.host(None, K, want_pairs)
    for key, v in (("first_step", -1), ("first_partner", -1), ("min_d2", np.inf), ("pair_first", -1)):
        if key in rows:
            rows[key][...] = v
    return rows, o


class PolyTrajSet:
    """K solved trajectories on the device (mplx_poly of include/mplx_solve.h): what EnvMap.solve_traj returns and what
    EnvMap.solve_traj_resident solves into.  status [K] (SOLVE_EMPTY | SOLVE_BAD_TIME | SOLVE_SINGULAR; 0 = solved);
    a failed problem has no samples and traverses as an empty trajectory.  free() it before the EnvMap is closed."""

    def __init__(self, env, k_cap, w_max):
        self._env, self.k_cap, self.w_max = env, int(k_cap), int(w_max)
        self.n, self.so, self.n_wmax, self.control = 0, None, 0, None
        self._host, self._out, self._lambda = None, None, None
        h = C.c_void_p()
        _abi.check(env._ctx, _abi.lib().mplx_poly_create(env._ctx, self.k_cap, self.w_max, C.byref(h)))
        self._h = h

    def free(self):
        if self._h is not None and self._env._ctx:
            _abi.lib().mplx_poly_destroy(self._h)
        self._h = None
        if self._out is not None:
            self._out.free()
            self._out = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _check(self, rc):
        _abi.check(self._env._ctx, rc)

    def _rows(self):
        """The rows of the last solve or load on the host: from the host-pointer call, or downloaded from the SolveOut /
        LoadOut of the resident one."""
        if self._host is None:
            if self._out is None:
                raise RuntimeError("PolyTrajSet: the resident solve or load kept no output rows (no `out` was given)")
            self._env.synchronize()
            d = self._out.download()
            ok = d["status"] == 0
            d["n_segs"] = np.where(ok, d["n_segs"], 0)
            d["total_time"] = np.where(ok, d["total_time"], 0.0)
            if "coeff" in d:  # a SolveOut
                seg = np.arange(self._out.w_max - 1)[:, None] < d["n_segs"][None, :]
                d["coeff"] = np.where(seg[:, None, None, :], d["coeff"], 0.0)
                d["dts"] = np.where(seg, d["dts"], 0.0)
                d["yaw_coeff"] = np.where(seg[:, None, :], d["yaw_coeff"], 0.0)
            d["taus"] = np.where((np.arange(self._out.w_max)[:, None] <= d["n_segs"][None, :]) & ok[None, :], d["taus"], 0.0)
            self._host = d
        return self._host

    @property
    def status(self):
        return self._rows()["status"]

    @property
    def n_segs(self):
        return self._rows()["n_segs"]

    @property
    def total_time(self):
        return self._rows()["total_time"]

    def coefficients(self):
        """PolyTraj::p() of every problem: [w_max - 1][N][D][K], coefficient r of axis i of segment s at [s][r][i][k]
        (increasing powers of the segment's own time); zero past S_k and for a failed problem.  A solved set only."""
        if "coeff" not in self._rows():
            raise RuntimeError("PolyTrajSet: a loaded set has segments(), not the solver's coefficients()")
        return self._rows()["coeff"]

    def yaw_coefficients(self):
        """The yaw solve's p: [w_max - 1][2][K].  A solved set only."""
        if "yaw_coeff" not in self._rows():
            raise RuntimeError("PolyTrajSet: a loaded set has segments(), not the solver's yaw_coefficients()")
        return self._rows()["yaw_coeff"]

    def segments(self):
        """The primitives of every problem as EnvMap.load_traj takes them: [w_max - 1][D + 1][6][K], c(0) .. c(5) of
        primitive.h:128-131 for axis a of segment s at [s][a][:][k], axis D the yaw primitive; zero past S_k.  A loaded set
        returns what was loaded; a solved set PolyTraj::toPrimitives of its coefficients (c_j = p_{5-j} (5-j)!, the
        multiplication the device made)."""
        r = self._rows()
        if "segments" not in r and "coeff" not in r:
            raise RuntimeError("PolyTrajSet: a set loaded with load_traj_resident keeps its dts and segments on the device only")
        if "segments" not in r:
            p, yaw = r["coeff"], r["yaw_coeff"]
            S, N, D, K = p.shape
            seg = np.zeros((S, D + 1, 6, K))
            fact = [1.0, 1.0, 2.0, 6.0, 24.0, 120.0]
            for j in range(6):
                if 5 - j < N:
                    seg[:, :D, j, :] = p[:, 5 - j, :, :] * fact[5 - j]
            seg[:, D, 4, :], seg[:, D, 5, :] = yaw[:, 1, :] * 1.0, yaw[:, 0, :] * 1.0
            r["segments"] = seg
        return r["segments"]

    def dts(self):
        """[w_max - 1][K] segment durations (given, or allocate_time's); zero past S_k.  Not for a set loaded from
        device buffers (load_traj_resident): its segments and durations are the caller's own arrays."""
        if "dts" not in self._rows():
            raise RuntimeError("PolyTrajSet: a set loaded with load_traj_resident keeps its dts and segments on the device only")
        return self._rows()["dts"]

    def taus(self):
        """[w_max][K]: taus[0 .. S_k] by sequential addition of dts."""
        return self._rows()["taus"]

    def _need(self):
        if self._h is None or self.n == 0:
            raise RuntimeError("PolyTrajSet: nothing solved (or freed)")
        self._env._flush()

    def info(self, want_states=False):
        """status, n_segs, total_time, effort [5][K] = J(VEL), J(ACC), J(JRK), J(SNP), Jyaw of the solved primitives;
        want_states: seg_state [4D+2][w_max][K], the waypoints (mplx_poly_info; synchronous)."""
        self._need()
        out, o = TrajInfo.host(self._env, self.n, self.n_wmax - 1, want_states)
        self._check(_abi.lib().mplx_poly_info(self._h, C.byref(o)))
        return out

    def sample(self, N=None, times=None, form=TRAJ_COMMAND, out=None):
        """As EnvMap.traj_sample on the solved set (mplx_poly_sample; synchronous): samples [4D+3][K][count], status."""
        self._need()
        K, env = self.n, self._env
        t, tkeep, count = env._traj_times(N, times, form, K)
        rows = 4 * env.dim + 3
        if out is None:
            out = np.zeros((rows, K, max(count, 0)), np.float64)
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.ndim != 3 or out.shape[0] != rows or out.shape[1] < K:
            raise ValueError("out must be a C-contiguous float64 [%d][>= K][count']" % rows)
        status = np.zeros(K, np.uint8)
        o = _abi.TrajSampleOut()
        o.out, o.row_stride, o.sample_stride, o.status = out.ctypes.data, out.shape[1] * out.shape[2], out.shape[2], status.ctypes.data
        self._check(_abi.lib().mplx_poly_sample(self._h, C.byref(t), C.byref(o)))
        return {"samples": out, "status": status}

    def traverse(self, lanes=0):
        """As EnvMap.traj_traverse on the solved set, on the maps the device holds now (mplx_poly_traverse)."""
        self._need()
        out, o = TrajTraverse.host(self._env, self.n)
        self._check(_abi.lib().mplx_poly_traverse(self._h, int(lanes), C.byref(o)))
        return out

    def limits(self, v_max=None, a_max=None, j_max=None, all_roots=False):
        """Primitive::max_vel / max_acc / max_jrk and validate_primitive of every trajectory (mplx_poly_limits;
        synchronous).  Limits default to the EnvMap's; <= 0 means not checked.  all_roots=False is the reference, which
        stops at the first root past the segment's end and so often misses the true peak; all_roots=True looks at every
        root (include/mplx_limits.h).  Returns max_vel / max_acc / max_jrk [D][K] (per axis, the maximum over the
        segments), exceed [K] (EXCEED_VEL | EXCEED_ACC | EXCEED_JRK), valid [K] (under the set's control) and first_bad
        [K] (segment or -1); entries of failed problems are zero (valid 0, first_bad -1)."""
        self._need()
        out, o = PolyLimits.host(self._env, self.n)
        out["first_bad"][:] = -1
        self._check(_abi.lib().mplx_poly_limits(self._h, C.byref(self._limits_in(v_max, a_max, j_max, all_roots)), C.byref(o)))
        return out

    def _limits_in(self, v_max, a_max, j_max, all_roots):
        p, i = self._env._p, _abi.LimitsIn()
        i.mv = float(p.v_max if v_max is None else v_max)
        i.ma = float(p.a_max if a_max is None else a_max)
        i.mj = float(p.j_max if j_max is None else j_max)
        i.mode = _abi.LIMITS_ALL_ROOTS if all_roots else _abi.LIMITS_REFERENCE
        return i

    # asynchronous forms on HBM-resident rows (rows.TrajInfo / TrajSamples / TrajTraverse); synchronize() before reading
    def limits_resident(self, out, v_max=None, a_max=None, j_max=None, all_roots=False):
        """out: EnvMap.alloc_poly_limits(n)."""
        self._need()
        o = out.c_struct()
        self._check(_abi.lib().mplx_poly_limits_device(self._h, C.byref(self._limits_in(v_max, a_max, j_max, all_roots)), C.byref(o)))

    def info_resident(self, out):
        self._need()
        o = out.c_struct()
        self._check(_abi.lib().mplx_poly_info_device(self._h, C.byref(o)))

    @staticmethod
    def _device_times(N, times, n_times, time_stride, form=TRAJ_COMMAND):
        t = _abi.TrajTimes()
        t.form = int(form)
        if N is not None:
            t.n_uniform = int(N)
        else:
            t.times, t.n_times, t.time_stride = _device_ptr(times), int(n_times), int(time_stride)
        return t

    def sample_resident(self, out, N=None, times=None, n_times=None, time_stride=0, form=TRAJ_COMMAND):
        self._need()
        t = self._device_times(N, times, n_times, time_stride, form)
        o = out.c_struct()
        self._check(_abi.lib().mplx_poly_sample_device(self._h, C.byref(t), C.byref(o)))

    def traverse_resident(self, out, lanes=0):
        self._need()
        o = out.c_struct()
        self._check(_abi.lib().mplx_poly_traverse_device(self._h, int(lanes), C.byref(o)))

    # ---- conflicts between the trajectories of the set on a common clock (include/mplx_conflict.h)
    def conflicts(self, step, n_steps=None, t0=None, radius=None, group=None, rank=None, park=True, want_pairs=False, chunk_steps=0):
        """Which trajectories come closer than the sum of their radii, when first and with whom (mplx_poly_conflicts;
        synchronous).  Instant i is at i * step on a clock on which trajectory k starts at t0[k] (None: 0); positions are
        those of sample() at i * step - t0[k].  n_steps=None: the smallest count that covers max(t0 + total), from the
        totals on the host.  radius: a scalar or [K].  group [K]: trajectories of one group never conflict (the n_v
        candidates of one robot in the Q x n_v layout of smooth(v=[...])).  rank [K]: a conflict is charged to a only if
        rank[b] <= rank[a] (the larger rank yields, equal ranks both do); None: to both.  park=True: a robot waits at its
        start before t0 and at its end afterwards; False: it exists only during its own trajectory.  chunk_steps: the
        instants per pass, 0 automatic; no result depends on it.  Returns a ConflictResult."""
        self._need()
        K = self.n
        if n_steps is None:
            inf = self.info()
            n_steps = _conflict_steps(float(step), t0, inf["total_time"], inf["status"] == 0)
        i, keep = _conflict_in(K, step, n_steps, t0, radius, group, rank, park, chunk_steps, False)
        rows, o = _conflict_host_out(K, want_pairs)
        self._check(_abi.lib().mplx_poly_conflicts(self._h, C.byref(i), C.byref(o)))
        return ConflictResult(step, rows["first_step"], rows["first_partner"], rows["min_d2"], rows["status"], rows.get("pair_first"))

    def conflicts_resident(self, out, step, n_steps, t0=None, radius=None, group=None, rank=None, park=True, chunk_steps=0):
        """Asynchronous (mplx_poly_conflicts_device).  out: EnvMap.alloc_conflicts(n, want_pairs); t0 / radius / group /
        rank: device buffers of [K] (radius may be a scalar) or None; n_steps must be given: nothing is read back."""
        self._need()
        i, keep = _conflict_in(self.n, step, n_steps, t0, radius, group, rank, park, chunk_steps, True)
        o = out.c_struct()
        self._check(_abi.lib().mplx_poly_conflicts_device(self._h, C.byref(i), C.byref(o)))

    # ---- time scaling (include/mplx_scale.h): a Lambda per problem.  robust=False is the reference with its quirks (the
    # 1e-5 clamp of its coefficients, a getTau that loses the end points); robust=True validates the points, applies
    # no clamp and inverts the time map by Newton steps.  Afterwards sample() takes real times, info() reports the
    # scaled total and traverse() is refused until clear_lambda().
    def _lambda_host(self, count=0):
        """The host twin of LambdaRows for this set: its c_struct / c_down / c_tau and _host_rows(group)."""
        return LambdaRows._host(self._env, self.n, self.n_wmax, count)

    def _keep_lambda(self, rows):
        self._lambda = {k: rows[k] for k in ("status", "n_lseg", "total", "Ts", "segs")}
        return rows

    @staticmethod
    def _mode(robust):
        return _abi.SCALE_ROBUST if robust else _abi.SCALE_REFERENCE

    def _scale_in(self, ri, rf, robust, keep):
        i = _abi.ScaleIn()
        i.mode = self._mode(robust)
        for name, v in (("ri", ri), ("rf", rf)):
            if np.ndim(v) == 0:
                setattr(i, name, float(v))
            else:
                a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.n,)))
                keep.append(a)
                setattr(i, name + "_arr", a.ctypes.data)
        return i

    def scale(self, ri, rf, robust=True):
        """Trajectory::scale(ri, rf) on every trajectory (mplx_poly_scale; synchronous): ri, rf scalars or [K] ratios at
        the start and the end.  Returns status [K] (0, LAMBDA_BAD_POINTS, LAMBDA_NOT_POSITIVE), n_lseg, total, Ts, segs;
        entries of failed problems are zero."""
        self._need()
        keep = []
        h = self._lambda_host()
        o = h.c_struct()
        i = self._scale_in(ri, rf, robust, keep)
        self._check(_abi.lib().mplx_poly_scale(self._h, C.byref(i), C.byref(o)))
        return self._keep_lambda(h._host_rows("out"))

    def _down_in(self, v_max, a_max, ri, rf, robust):
        p, i = self._env._p, _abi.ScaleDownIn()
        i.mv = float(p.v_max if v_max is None else v_max)
        i.ma = float(p.a_max if a_max is None else a_max)
        i.ri, i.rf, i.mode = float(ri), float(rf), self._mode(robust)
        return i

    def scale_down(self, v_max=None, a_max=None, ri=0.0, rf=0.0, robust=True):
        """Slow every trajectory that breaks v_max / a_max (default: the EnvMap's; <= 0: not checked) down to them
        (mplx_poly_scale_down; synchronous).  ri, rf: lambda at the two ends, <= 0: max_l, i.e. no ramp; with both the
        scaling is uniform and within the limits by construction -- ramps are NOT checked against the limits.  Returns
        scaled [K] (0: within the limits, left unscaled), max_l, t_lo, t_hi and the rows of scale()."""
        self._need()
        h = self._lambda_host()
        o = h.c_down()
        i = self._down_in(v_max, a_max, ri, rf, robust)
        self._check(_abi.lib().mplx_poly_scale_down(self._h, C.byref(i), C.byref(o)))
        return self._keep_lambda({**h._host_rows("out"), **h._host_rows("down")})

    @staticmethod
    def _points(p, v, t, K):
        """[9][3][K] rows of p, v, t given as [n_max][K] (or [n_max]: the same for every problem)."""
        cols = [np.asarray(x, dtype=np.float64) for x in (p, v, t)]
        cols = [np.broadcast_to(x[:, None], (x.shape[0], K)) if x.ndim == 1 else x for x in cols]
        n_max = cols[0].shape[0]
        if n_max > 9 or any(x.shape != (n_max, K) for x in cols):
            raise ValueError("p, v, t must be [n <= 9][K] (or [n <= 9])")
        pts = np.zeros((9, 3, K))
        for f, x in enumerate(cols):
            pts[:n_max, f, :] = x
        return pts, n_max

    def set_lambda(self, p, v, t, n_pts=None, robust=True):
        """Lambda(vs) from virtual points (mplx_poly_set_lambda; synchronous): p, v, t [n_max][K] (or [n_max]), point j of
        problem k at [j][k], j < n_pts[k] (None: n_max each).  Returns the rows of scale()."""
        self._need()
        K = self.n
        pts, n_max = self._points(p, v, t, K)
        n = np.ascontiguousarray(np.broadcast_to(np.asarray(n_max if n_pts is None else n_pts, dtype=np.int32), (K,)))
        h = self._lambda_host()
        o = h.c_struct()
        i = _abi.LambdaIn()
        i.pts, i.stride, i.n_pts, i.mode = pts.ctypes.data, K, n.ctypes.data, self._mode(robust)
        self._check(_abi.lib().mplx_poly_set_lambda(self._h, C.byref(i), C.byref(o)))
        return self._keep_lambda(h._host_rows("out"))

    def clear_lambda(self):
        """Every trajectory is unscaled again."""
        self._need()
        self._check(_abi.lib().mplx_poly_clear_lambda(self._h))
        self._lambda = None

    def _lambda_rows(self):
        rows = self._lambda
        if rows is None:
            raise RuntimeError("PolyTrajSet: no Lambda (scale, scale_down or set_lambda first; the _resident forms keep theirs on the device)")
        return rows

    def lambda_segments(self):
        """The Lambda of every problem as the last synchronous scale / scale_down / set_lambda left it: a [8][4][K] (a3 a2
        a1 a0 of segment s at [s][:][k]), ti, tf, T0 (getT(ti)), dT [8][K], n_lseg [K], status [K]."""
        r = self._lambda_rows()
        g = r["segs"]
        return {"a": g[:, 0:4, :], "ti": g[:, 4, :], "tf": g[:, 5, :], "T0": g[:, 6, :], "dT": g[:, 7, :], "n_lseg": r["n_lseg"],
                "status": r["status"]}

    def segment_times(self):
        """Trajectory::getSegmentTimes: [w_max - 1][K], Ts[s + 1] - Ts[s]; zero past S_k and for a problem without a
        Lambda status 0."""
        r = self._lambda_rows()
        Ts = r["Ts"]
        ok = (np.arange(self.n_wmax - 1)[:, None] < self.n_segs[None, :]) & (r["n_lseg"] > 0)[None, :]
        return np.where(ok, Ts[1:] - Ts[:-1], 0.0)

    def tau(self, times=None, N=None):
        """The inverse time map (mplx_poly_tau; synchronous): tau, lambda, lambda_dot [K][count] and found [K][count] at
        the real times `times` ([Q] or [K][Q]) or at the N + 1 uniform ones."""
        self._need()
        t, tkeep, count = self._env._traj_times(N, times, TRAJ_COMMAND, self.n)
        h = self._lambda_host(count)
        o = h.c_tau()
        self._check(_abi.lib().mplx_poly_tau(self._h, C.byref(t), C.byref(o)))
        return h._host_rows("tau")

    # asynchronous forms on HBM-resident rows (EnvMap.alloc_lambda_rows); synchronize() before reading
    def scale_resident(self, out, ri, rf, robust=True):
        """ri, rf: scalars, or DeviceArrays of [K] float64."""
        self._need()
        i = _abi.ScaleIn()
        i.mode = self._mode(robust)
        for name, v in (("ri", ri), ("rf", rf)):
            if np.ndim(v) == 0 and not hasattr(v, "ptr") and not hasattr(v, "data_ptr"):
                setattr(i, name, float(v))
            else:
                setattr(i, name + "_arr", _device_ptr(v))
        o = out.c_struct()
        self._check(_abi.lib().mplx_poly_scale_device(self._h, C.byref(i), C.byref(o)))
        self._lambda = None

    def scale_down_resident(self, out, v_max=None, a_max=None, ri=0.0, rf=0.0, robust=True):
        self._need()
        o = out.c_down()
        i = self._down_in(v_max, a_max, ri, rf, robust)
        self._check(_abi.lib().mplx_poly_scale_down_device(self._h, C.byref(i), C.byref(o)))
        self._lambda = None

    def set_lambda_resident(self, out, pts, n_pts=None, stride=None, robust=True):
        """pts: [9][3][stride] float64 on the device; n_pts: [K] int32 on the device or None (9 each)."""
        self._need()
        i = _abi.LambdaIn()
        i.pts, i.stride, i.mode = _device_ptr(pts), self.n if stride is None else int(stride), self._mode(robust)
        if n_pts is not None:
            i.n_pts = _device_ptr(n_pts)
        o = out.c_struct()
        self._check(_abi.lib().mplx_poly_set_lambda_device(self._h, C.byref(i), C.byref(o)))
        self._lambda = None

    def tau_resident(self, out, N=None, times=None, n_times=None, time_stride=0):
        """out: alloc_lambda_rows(n, w_max, count) with count >= the sample count."""
        self._need()
        t = self._device_times(N, times, n_times, time_stride, 0)
        o = out.c_tau()
        self._check(_abi.lib().mplx_poly_tau_device(self._h, C.byref(t), C.byref(o)))
