// lists_route.cpp -- mplx_expand_lists_device* (include/mplx.h): per-node successor lists on device buffers.  Three
// routes produce the same lists: GRID (the factorised kernels expand_grid / expand_lex / expand_pair_kernel.hip), TILE
// (expand_tile_kernel.hip) and DENSE (expand_kernel.hip into scratch + ordered compaction).  This unit holds the plans
// that decide which route covers a configuration and how its launch is sized, the tables the routes read (blocked
// bits, free-box table, sample times), the builders of the kernels' argument blocks and the dispatch itself.
#include "mplx_ctx.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>

namespace mplx_detail {

// ---------------------------------------------------------------- argument blocks
// ExpandArgs, TileArgs, GridArgs and CompactArgs name their common fields alike: one copy of each group.

// the environment: map extents, origin, resolution, search region, time step, weight and limits
template <class Args>
static void set_env(const mplx_ctx *c, Args *a) {
  a->region = c->has_region ? (const uint32_t *)c->region_bits.p : nullptr;
  a->dim0 = c->mdim[0]; a->dim1 = c->mdim[1]; a->dim2 = c->mdim[2];
  a->org0 = c->origin[0]; a->org1 = c->origin[1]; a->org2 = c->origin[2];
  a->res = c->res;
  a->dt = c->prm.dt; a->w = c->prm.w;
  a->v_max = c->prm.v_max; a->a_max = c->prm.a_max; a->j_max = c->prm.j_max;
}

// the tables of ensure_tables (the dense kernel's ExpandArgs has none)
template <class Args>
static void set_tables(const mplx_ctx *c, Args *a) {
  a->ttab = (const double *)c->tables.p;
  a->tcnt = (const unsigned char *)c->tables.p + kTcntOffset;
  a->Rres = c->recips[0]; a->R001 = c->recips[1]; a->R01 = c->recips[2];
}

// the rows of the lists
template <class Args>
static void set_lists(const mplx_ctx *c, const mplx_succ_lists *o, Args *a) {
  a->l_count = o->count; a->l_action = o->action; a->l_cost = o->cost; a->l_hash = o->hash;
  a->l_state = o->state; a->l_stride = o->state_stride; a->l_iters = o->iters;
  a->l_nstride = list_stride(c, o);
}

mplx::ExpandArgs expand_args(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                             const mplx_succ *o) {
  mplx::ExpandArgs a{};
  set_env(c, &a);
  a.map = (const int8_t *)c->map.p;
  a.pot = c->has_pot ? (const int8_t *)c->pot.p : nullptr;
  a.wyaw = c->prm.wyaw; a.yaw_max = c->prm.yaw_max;
  a.pot_w = c->prm.potential_weight; a.grad_w = c->prm.gradient_weight;
  a.U = (const double *)c->U.p;
  a.nU = c->nU; a.udim = c->udim;
  a.nodes = d_nodes; a.n_nodes = n_nodes; a.node_stride = node_stride;
  a.status = o->status; a.cost = o->cost; a.hash = o->hash; a.state = o->state;
  a.state_stride = o->state_stride; a.iters = o->iters;
  return a;
}

// the goal of mplx_set_goal with this launch's output rows (null rows: nothing is computed)
static mplx::PostFuse post_of(const mplx_ctx *c, const mplx_succ_lists *o) {
  mplx::PostFuse f = c->goal_fuse;
  f.heur = o->heur;
  f.flags = o->flags;
  return f;
}

mplx::TileArgs tile_args(mplx_ctx *c, const TilePlan &tp, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                         const mplx_succ_lists *o) {
  mplx::TileArgs a{};
  set_env(c, &a);
  set_tables(c, &a);
  set_lists(c, o, &a);
  a.map = (const int8_t *)c->map.p;
  a.U = (const double *)c->U.p;
  a.nU = c->nU; a.udim = c->udim;
  a.inv_nU = 1.0f / (float)c->nU;
  a.nodes = d_nodes; a.n_nodes = n_nodes; a.node_stride = node_stride;
  a.npb = tp.npb; a.tile_pairs = tp.tile_pairs; a.wl_cap = tp.wl_cap; a.n_max = tp.n_max;
  a.lds_u_offset = tp.u_offset; a.grid_limit = tp.grid;
  a.dbg = c->tune.dbg;  // timing ablations, 0 in production
  a.post = post_of(c, o);
  return a;
}

// The completion word of a launch whose caller waits for it on the spot (mplx_ctx::want_done; DoneSignal).  The caller
// sets done_armed once the launch is in.
static void arm_done(mplx_ctx *c, mplx::DoneSignal *done) {
  c->done_armed = false;
  if (c->want_done && c->tune.done_flag && c->done_host) {
    done->flag = c->done_host;
    done->count = (uint32_t *)c->done_count.p;
    done->seq = ++c->done_seq;
  }
}

// ---------------------------------------------------------------- plans
// Largest per-pair sample count a kernel has to serve, or 0 where it is unbounded or above `limit`: a valid pair has
// max_v <= v_max (primitive.h:483-496), and for plain VEL control max_v = max |u|.
static int sample_bound(const mplx_ctx *c, double limit) {
  const mplx_params &p = c->prm;
  double vbound;
  if ((p.control & 0x0f) == MPLX_VEL) vbound = c->u_absmax;
  else if (p.v_max > 0) vbound = p.v_max;
  else return 0;                               // unbounded sample count
  const double nf = std::ceil(vbound * p.dt / c->res) + 1.0;  // +1: slack for the last rounding
  if (!(nf <= limit)) return 0;
  const int n_max = (int)nf;
  return n_max < 5 ? 5 : n_max;
}

// Decide whether the tiled kernel covers the current configuration and how to
// tile it.  The work-list capacity needs a bound on the per-pair sample count.
TilePlan plan_tile(const mplx_ctx *c) {
  TilePlan t;
  const mplx_params &p = c->prm;
  if (p.control & 0x10) return t;              // yaw: per-sample costs, dense kernel
  if (c->has_pot) return t;                    // potential: per-sample costs, dense kernel
  if (c->nU > 1024 || c->nU < 1) return t;
  const int n_max = sample_bound(c, 63.0);
  if (!n_max) return t;
  const int cnt_max = n_max + 1;               // the loop runs n or n+1 times
  int npb = 1024 / c->nU;
  if (npb < 1) npb = 1;
  if (npb > 32) npb = 32;
  for (; npb >= 1; npb--) {
    const int tp = npb * c->nU;
    int uoff = 0;
    const size_t lds = mplx::tile_lds_bytes(tp, npb, tp * cnt_max, n_max, 4 * c->dim + 2, c->nU * c->udim, &uoff);
    if (lds <= 80 * 1024 || npb == 1) {   // at least two 512-thread workgroups per CU (160 KiB LDS)
      if (lds > kLdsBudget - 64) return t;  // (- 64: the service form's static command word)
      t.ok = true;
      t.npb = npb;
      t.tile_pairs = tp;
      t.wl_cap = tp * cnt_max;
      t.n_max = n_max;
      t.u_offset = uoff;
      t.grid = c->n_cus * (lds <= 53 * 1024 ? 3 : lds <= 80 * 1024 ? 2 : 1);
      return t;
    }
  }
  return t;
}

namespace {
struct GridPlan {
  bool ok = false;
  int ndp = 1, n_max = 0, rmax = 0, boxcap = 0, grid = 0, order = 0;
  int ulex = 0;      // = GridArgs::ulex
  bool gather = false, use_sat = true;
  bool lex = false;  // expand_lex_kernel.hip serves it (lexicographic table, no yaw, occupancy map)
};
struct PairPlan {    // expand_pair_kernel.hip takes the launch: rows per pass and workgroups
  bool ok = false;
  int rmax = 0, grid = 0;
};
// the kernels of the GRID route in the key of the context's occupancy cache: bits 8-9 of its control word
enum OccKernel { kOccGrid = 0, kOccLex = 0x100, kOccPair = 0x200 };
}  // namespace

// Workgroups of one kernel instantiation that are resident per CU with `lds` bytes each; 0: more than a CU has.
// The launches of this route are persistent: every workgroup must be RESIDENT (a workgroup that waits for a slot starts
// its first, statically assigned node only after another one has drained the whole queue).  What fits is the runtime's
// answer for this instantiation (registers, LDS granules), not LDS bytes alone; it is asked once and cached per
// (kernel, control, inst, potential, LDS).  inst: what selects the instantiation besides the control flag (bits 12+ of
// the key) -- the lexicographic kernel's table size by the values per axis, the pair kernel's yaw rates.
static int resident_per_cu(const mplx_ctx *c, OccKernel kernel, int inst, int rows_per_pass, size_t lds) {
  if (lds > kLdsBudget) return 0;
  const int control = c->prm.control, key = control | kernel | (inst << 12);
  int nb = -1;
  for (const auto &e : c->grid_occ)
    if (e.control == key && e.pot == c->has_pot && e.lds == lds) nb = e.nb;
  if (nb < 0) {
    nb = kernel == kOccLex    ? mplx::lex_resident_blocks(c->dim, control, inst, lds)
         : kernel == kOccPair ? mplx::pair_resident_blocks(c->dim, control, inst, lds)
                              : mplx::grid_resident_blocks(c->dim, control, c->has_pot, lds);
    if (c->grid_occ.size() >= 8) c->grid_occ.clear();
    c->grid_occ.push_back({key, c->has_pot, lds, nb});
    if (getenv("MPLX_GRID_VERBOSE"))
      fprintf(stderr, "mplx: %s kernel control 0x%x pot %d rows/pass %d: LDS %zu B per workgroup, %d workgroups resident per CU\n",
              kernel == kOccLex ? "lex" : kernel == kOccPair ? "pair" : "grid", control, (int)c->has_pot, rows_per_pass, lds, nb);
  }
  const int by_lds = (int)(kLdsBudget / lds);
  return (nb > 0 && nb < by_lds) ? nb : by_lds;
}

// Does the factorised kernel cover the current configuration, and how is it sized?
static GridPlan plan_grid(const mplx_ctx *c) {
  GridPlan g;
  const mplx_params &p = c->prm;
  const bool yaw = (p.control & 0x10) != 0;
  if (yaw && (c->udim != c->dim + 1 || c->u_nd[3] < 1)) return g;
  if (!c->u_factored || c->nU < 1) return g;
  // (control tables of more than 1 024 entries or more than 16 values on an axis: the lexicographic kernel alone, up to 8 192)
  const bool lex_only = c->u_wide || c->nU > 1024;
  if (lex_only && (c->nU > 8192 || !c->u_lex || c->tune.no_lex || !c->tune.grid_lex || yaw || c->has_pot ||
                   !mplx::lex_covers(c->dim, p.control)))
    return g;
  const int n_max = sample_bound(c, 61.0);
  if (!n_max) return g;
  int ndp = 1;
  for (int i = 0; i < c->dim; i++) ndp = c->u_nd[i] > ndp ? c->u_nd[i] : ndp;
  // LDS per wave: `rmax` rows of cell codes per axis entry and `boxcap` dwords of staged blocked bits.
  // A box of (n_max + 3)^(D-1) rows covers every node whose per-axis velocities keep their sign.
  const int order = control_order(p.control);
  // (SNP: the rare primitives whose cell codes leave their range are sampled by direct evaluation, which covers
  // potential maps and the heading cost too since round 3)
  // GridLds's mode word: bits 0-1 the yaw tables, bit 2 the velocity rows of every axis (gradient cost of a potential map)
  const int ym = (yaw ? (p.wyaw > 0 ? 2 : 1) : 0) | ((c->has_pot && p.gradient_weight != 0) ? 4 : 0), ndy = yaw ? c->u_nd[3] : 0;
  int rmax = 4, boxcap = (c->dim == 3) ? (n_max + 3) * (n_max + 3) : 4 * (n_max + 3);
  if (boxcap < 64) boxcap = 64;
  if (boxcap > 1024) boxcap = 1024;
  if (c->has_pot) boxcap = 64;  // potential maps are sampled from the int8 map itself: no staged bits (LDS buys occupancy)
  // Gather mode (the sample loops read the blocked-bit map directly instead of staging the reach box in LDS): fewer
  // look-ups than box rows for small control tables, yet slower in practice -- a look-up costs 35 instructions
  // against 17 from LDS.
  g.gather = false;  // measured slower than staging on C2 / C3 (profiles/README.md round 2): kept as a forced mode
  if (c->tune.grid_gather >= 0) g.gather = c->tune.grid_gather != 0;
  // Free-box query: exact reach boxes exist for K <= 2; for K = 3 the box is the conservative |p - p0| <= max_vel * T,
  // rarely free, and the query is one more dependent round trip per node (C3: -6 % without it)
  g.use_sat = (!g.gather || c->has_pot) && order <= 2;
  if (c->tune.grid_sat >= 0) g.use_sat = c->tune.grid_sat != 0;
  if (g.gather) boxcap = 64;
  if (c->tune.grid_rmax > 0) rmax = c->tune.grid_rmax;
  if (c->tune.grid_boxcap > 0) boxcap = c->tune.grid_boxcap;
  if (rmax < 1) rmax = 1;
  // (a table with a yaw-rate column under a flag without yaw is nested-loop order over FOUR factors, and the kernels
  // enumerate three then: such a table goes through its per-control indices)
  const int ulex = (c->u_lex && !c->tune.no_lex && (yaw || c->udim == c->dim)) ? 1 : 0;
  // the lexicographic kernel: same plan, its own LDS carve-up and occupancy
  g.lex = ulex && !yaw && !c->has_pot && !g.gather && c->tune.grid_lex && mplx::lex_covers(c->dim, p.control);
  if (lex_only && !g.lex) return GridPlan();
  auto lds_of = [&](int rm) -> size_t {
    return g.lex ? mplx::lex_lds_bytes(c->dim, order, ndp, c->nU, n_max, rm, boxcap)
                 : mplx::grid_lds_bytes(c->dim, order, c->nU, ndp, n_max, rm, boxcap, ym, ndy, ulex);
  };
  while (rmax > 1 && lds_of(rmax) > 80 * 1024) rmax--;
  // (both factorised kernels run 4 waves = 4 nodes in flight per workgroup; plan_grid, grid_work and the prescreen
  // threshold size launches with the one figure)
  const int wpb = g.lex ? mplx::lex_waves_per_block() : mplx::grid_waves_per_block();
  if (mplx::lex_waves_per_block() != mplx::grid_waves_per_block()) return GridPlan();
  // every workgroup of the launch must be resident: the runtime's answer for this instantiation (resident_per_cu)
  auto resident = [&](int rm, size_t *lds_out) -> int {
    *lds_out = lds_of(rm);
    return g.lex ? resident_per_cu(c, kOccLex, ndp, rm, *lds_out) : resident_per_cu(c, kOccGrid, 0, rm, *lds_out);
  };
  // 16 waves per CU (4 per SIMD): what the register allocation of every instantiation allows, and the measured
  // optimum where more would fit (profiles/README.md)
  // (the lexicographic kernel is leaner and latency-bound: C4 edges-only 0.353 / 0.302 / 0.278 ms at 12 / 16 / 20 waves per
  // CU, profiles/r04_lex_occupancy.txt -- it takes what its registers and LDS allow, up to 24)
  const int cap = c->tune.grid_waves_per_cu > 0 ? c->tune.grid_waves_per_cu : (g.lex ? 24 : 16);
  size_t lds = 0;
  int per_cu = resident(rmax, &lds);
  if (per_cu < 1) return g;
  // A slightly smaller box budget when that admits another workgroup (lexicographic kernel, Dim 3): the staged box of a
  // node is (n_max + 3)^2 words at most and far smaller for nearly every node (the rare larger one reads the blocked-bit
  // map directly).  C3: 1024 -> 800 words = 4 instead of 3 workgroups per CU, 71.5 -> 65.4 us.
  if (g.lex && c->dim == 3 && c->tune.grid_boxcap <= 0 && per_cu * wpb < cap) {
    const int keep = boxcap;
    boxcap = (boxcap * 25 / 32) & ~31;
    size_t lds_b = 0;
    const int per_cu_b = boxcap >= 256 ? resident(rmax, &lds_b) : 0;
    if (per_cu_b > per_cu) { per_cu = per_cu_b; lds = lds_b; }
    else boxcap = keep;
  }
  // One row less per pass when that is what lets another workgroup in (the heading-cost tables of ACCxYAW with
  // wyaw > 0: 45 KB per workgroup = 3 resident, 35 KB = 4; C5 0.108 -> 0.103 ms, a second pass is rare)
  if (c->tune.grid_rmax <= 0 && rmax == 4 && per_cu * wpb < cap) {
    size_t lds3 = 0;
    const int per_cu3 = resident(3, &lds3);
    if (per_cu3 > per_cu) { rmax = 3; per_cu = per_cu3; lds = lds3; }
  }
  if (per_cu * wpb > cap) per_cu = cap / wpb;
  if (per_cu < 1) per_cu = 1;
  g.ok = true;
  g.ndp = ndp;
  g.n_max = n_max;
  g.rmax = rmax;
  g.boxcap = boxcap;
  g.order = order;
  g.ulex = ulex;
  g.grid = c->n_cus * per_cu;
  if (c->tune.grid_blocks > 0) g.grid = c->tune.grid_blocks;
  return g;
}

// Yaw controls on a potential map over a pre-screened frontier (BASELINE config 5): two nodes per wave
// (expand_pair_kernel.hip) -- the few thousand survivors then are ONE round of wave tasks instead of two.  Same lists.
// `a`: the launch as the factorised kernel would take it (pre-screen done, detection block set).
static PairPlan plan_pair(const mplx_ctx *c, const GridPlan &gp, const mplx::GridArgs &a) {
  PairPlan pp;
  if (!(a.live != nullptr && c->has_pot && a.ulex && !gp.lex && !c->tune.no_pair && a.yaw.tab == nullptr &&
        mplx::pair_covers(c->dim, c->prm.control) && c->dim * gp.ndp <= 16 && a.ndy <= mplx::pair_max_yaw_rates()))
    return pp;
  int per_cu = 0;
  for (int rm = c->tune.pair_rmax > 0 ? c->tune.pair_rmax : 3; rm >= 1 && per_cu < 1; rm--) {  // (rows per pass down to what fits at all)
    const size_t lds = mplx::pair_lds_bytes(c->dim, gp.order, c->nU, gp.ndp, gp.n_max, rm, c->prm.wyaw > 0, a.ndy);
    per_cu = resident_per_cu(c, kOccPair, a.ndy, rm, lds);
    pp.rmax = rm;
  }
  if (per_cu < 1) return pp;
  const int cap = c->tune.pair_wg_per_cu > 0 ? c->tune.pair_wg_per_cu : 3;  // 3 waves per SIMD: what its registers allow
  if (per_cu > cap) per_cu = cap;
  pp.grid = c->n_cus * per_cu;
  pp.ok = true;
  return pp;
}

// ---------------------------------------------------------------- launches of the GRID route
// Dynamic node assignment of the factorised kernel (GridArgs::work): two sets of counters in the context, used
// alternately; a launch finds its set zero and zeroes the other one for the next launch.
static int grid_work(mplx_ctx *c, mplx::GridArgs *a) {
  a->work = nullptr;
  a->work_zero = nullptr;
  a->work_chunk = 1;
  const int64_t wpb = mplx::grid_waves_per_block();
  const int64_t n_wg = (a->n_nodes + wpb - 1) / wpb;
  const int64_t W = (n_wg < (int64_t)a->grid_limit ? n_wg : (int64_t)a->grid_limit) * wpb;
  if (c->tune.grid_static || a->n_nodes <= W) return MPLX_OK;  // one node per wave at most: nothing to balance
  const size_t set_bytes = (size_t)mplx::kWorkCounters * 128;
  if (!c->work_counter.p) {
    if (int rc = ensure(c, c->work_counter, 2 * set_bytes)) return rc;
    HIP_TRY(c, hipMemsetAsync(c->work_counter.p, 0, 2 * set_bytes, c->stream));
    c->work_parity = 0;
  }
  a->work = (unsigned int *)((char *)c->work_counter.p + (c->work_parity ? set_bytes : 0));
  a->work_zero = (unsigned int *)((char *)c->work_counter.p + (c->work_parity ? 0 : set_bytes));
  // (the caller flips work_parity once the launch is enqueued: launch_grid below)
  // chunk: whole nodes per claim; 1 while a wave gets fewer than ~16 nodes (balance matters most), more beyond
  int64_t per_wave = a->n_nodes / W, ck = per_wave / 16;
  if (ck < 1) ck = 1;
  if (ck > 8) ck = 8;
  if (c->tune.grid_chunk > 0) ck = c->tune.grid_chunk;
  a->work_chunk = (int32_t)ck;
  a->work_blocked = c->tune.grid_blocked ? 1 : 0;
  return MPLX_OK;
}

// Enqueues the factorised kernel.  The counter sets change hands only when the launch went in: a launch that failed
// has not zeroed the other set, so the sets are dropped and made afresh (zeroed) on the next use.
int launch_grid(mplx_ctx *c, mplx::GridArgs *a) {
  if (int rc = grid_work(c, a)) return rc;
  const hipError_t e = a->lex ? mplx::launch_expand_lex(c->dim, c->prm.control, *a, c->stream)
                              : mplx::launch_expand_grid(c->dim, c->prm.control, *a, c->stream);
  c->last_grid_lex = a->lex != 0;
  c->last_grid_pair = false;
  if (e != hipSuccess) {
    if (a->work) {
      (void)hipStreamSynchronize(c->stream);
      release(c->work_counter);
    }
    return fail(c, MPLX_ERR_HIP, "expand_grid_kernel launch failed: %s", hipGetErrorString(e));
  }
  if (a->work) c->work_parity ^= 1;
  return MPLX_OK;
}

static int launch_pair(mplx_ctx *c, const PairPlan &pp, const mplx::GridArgs &a) {
  mplx::GridArgs b = a;
  b.rmax = pp.rmax;
  b.grid_limit = pp.grid;
  b.work = nullptr;
  b.work_zero = nullptr;
  const hipError_t e = mplx::launch_expand_pair(c->dim, c->prm.control, b, c->stream);
  if (e != hipSuccess) return fail(c, MPLX_ERR_HIP, "expand_pair_kernel launch failed: %s", hipGetErrorString(e));
  c->last_grid_lex = false;
  c->last_grid_pair = true;
  return MPLX_OK;
}

// Yaw controls with a heading limit on a frontier of several nodes per wave: validate_yaw(t = 0) of every node
// first, lane per node, and the main kernel walks the survivors only (grid_prescreen_kernel).  Small batches (a
// search's) skip it: one more launch costs them more than the dead nodes do.
static int prescreen(mplx_ctx *c, const GridPlan &gp, mplx::GridArgs *a) {
  const bool yaw = (c->prm.control & 0x10) != 0;
  const int64_t n_nodes = a->n_nodes;
  const int64_t ps_min = c->tune.prescreen_min > 0 ? c->tune.prescreen_min : (int64_t)4 * gp.grid * mplx::grid_waves_per_block();
  if (!(yaw && gp.order >= 2 && c->prm.yaw_max > 0 && c->tune.prescreen_min >= 0 && n_nodes >= ps_min && n_nodes < 0x7fffffffLL))
    return MPLX_OK;
  if (int rc = ensure(c, c->live_list, (size_t)n_nodes * 4)) return rc;
  // the survivors' counter: two words used alternately, each on its own line; a pre-screen launch finds its word
  // zero and zeroes the other one for the next launch of the stream (no memset per launch: it was 6.6 % of C5's GPU
  // time in round 3).  A launch that fails leaves the pair in an unknown state: dropped and made afresh.
  if (!c->live_ctr.p) {
    if (int rc = ensure(c, c->live_ctr, 256)) return rc;
    HIP_TRY(c, hipMemsetAsync(c->live_ctr.p, 0, 256, c->stream));
    c->live_parity = 0;
  }
  int32_t *live = (int32_t *)c->live_list.p;
  uint32_t *live_n = (uint32_t *)c->live_ctr.p + (c->live_parity ? 32 : 0);
  uint32_t *live_zero = (uint32_t *)c->live_ctr.p + (c->live_parity ? 0 : 32);
  const hipError_t pe = mplx::launch_grid_prescreen(c->dim, c->prm.control, *a, live, live_n, live_zero, c->stream);
  if (pe != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    release(c->live_ctr);
    return fail(c, MPLX_ERR_HIP, "grid_prescreen_kernel launch failed: %s", hipGetErrorString(pe));
  }
  c->live_parity ^= 1;
  a->live = live;
  a->live_n = live_n;
  return MPLX_OK;
}

// ---------------------------------------------------------------- tables
// (Re)build the summed-area table of the CURRENT blocked bits (new bits, or after mplx_edit_map patched them); it is
// skipped for maps where it would not fit an unsigned count or 16 GiB, and the kernel then samples every node.
static int rebuild_sat(mplx_ctx *c) {
  c->sat_stale = false;
  const int d2p = c->dim == 3 ? c->mdim[2] + 1 : 2;
  const int64_t sat_n = (int64_t)(c->mdim[0] + 1) * (c->mdim[1] + 1) * d2p;
  if (c->tune.no_sat || sat_n * 4 > (16LL << 30)) return MPLX_OK;
  if (int rc = ensure(c, c->sat, (size_t)sat_n * 4)) return rc;
  HIP_TRY(c, mplx::launch_build_sat(c->dim, (const uint32_t *)c->blk.p, c->mdim, (uint32_t *)c->sat.p, c->stream));
  c->sat_ok = true;
  return MPLX_OK;
}

int ensure_blocked_bits(mplx_ctx *c) {
  if (c->blk_ok) return MPLX_OK;
  c->sat_stale = false;
  const int64_t words = (c->n_cells + 31) >> 5;
  if (int rc = ensure(c, c->blk, (size_t)words * 4)) return rc;
  HIP_TRY(c, mplx::launch_build_blocked_bits((const int8_t *)(c->has_pot ? c->pot.p : c->map.p),
                                             c->has_region ? (const uint32_t *)c->region_bits.p : nullptr, c->n_cells,
                                             c->has_pot ? 1 : 0, (uint32_t *)c->blk.p, c->stream));
  c->sat_ok = false;  // the summed-area table for the free-box shortcut of the grid kernel goes with the bits
  if (int rc = rebuild_sat(c)) return rc;
  c->blk_ok = true;
  return MPLX_OK;
}

int ensure_tables(mplx_ctx *c) {
  if (c->tables_ok && c->tab_dt == c->prm.dt && c->tab_res == c->res) return MPLX_OK;
  const size_t bytes = kTcntOffset + 64 + 64;  // ttab, tcnt, 3 reciprocals (8-byte aligned tail)
  if (int rc = ensure(c, c->tables, bytes)) return rc;
  double *ttab = (double *)c->tables.p;
  unsigned char *tcnt = (unsigned char *)c->tables.p + kTcntOffset;
  double *rec = (double *)((unsigned char *)c->tables.p + kTcntOffset + 64);
  HIP_TRY(c, hipMemsetAsync(c->tables.p, 0, bytes, c->stream));
  HIP_TRY(c, mplx::launch_make_tables(c->prm.dt, c->res, ttab, tcnt, rec, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->recips, rec, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->tab_dt = c->prm.dt;
  c->tab_res = c->res;
  c->tables_ok = true;
  return MPLX_OK;
}

// ---------------------------------------------------------------- the three routes
// State rows a launch with this control can only fill with the literal +0.0 (bit f = row f of the 4D+2): the derivative
// rows of order above the control's, and the yaw row when the control carries no yaw (primitive.h:322).  From the
// control flags alone, hence the same for every launch of a search.
static uint32_t const_zero_rows(int dim, int control) {
  const int order = control_order(control);
  uint32_t m = 0;
  for (int b = order + 1; b <= 3; b++)
    for (int i = 0; i < dim; i++) m |= 1u << (b * dim + i);
  if (!(control & 0x10)) m |= 1u << (4 * dim);
  return m;
}

// The launch of the factorised kernels over the whole frontier, as plan_grid sized it (tables must be current: a.sat).
static mplx::GridArgs grid_args(mplx_ctx *c, const GridPlan &gp, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                                const mplx_succ_lists *o, uint32_t skip) {
  mplx::GridArgs a{};
  set_env(c, &a);
  set_tables(c, &a);
  set_lists(c, o, &a);
  a.blk = (const uint32_t *)c->blk.p;
  a.blk_words = (c->n_cells + 31) >> 5;
  a.pot = c->has_pot ? (const int8_t *)c->pot.p : nullptr;
  a.pot_w = c->prm.potential_weight;
  a.grad_w = c->has_pot ? c->prm.gradient_weight : 0.0;
  const bool yaw = (c->prm.control & 0x10) != 0;
  // the free-box shortcut skips the sample loops, which a per-sample heading cost (wyaw > 0) still needs
  a.sat = (c->sat_ok && gp.order <= 3 && !(yaw && c->prm.wyaw > 0) && !c->tune.no_sat && gp.use_sat)
              ? (const uint32_t *)c->sat.p : nullptr;
  a.gather = gp.gather ? 1 : 0;
  a.yaw_max = c->prm.yaw_max; a.wyaw = c->prm.wyaw; a.ndy = yaw ? c->u_nd[3] : 0;
  a.uvals = (const double *)c->uvals.p + (c->u_wide ? 4 * 16 : 0);
  a.uval_stride = c->u_wide ? 32 : 16;
  a.uidx = (const uint32_t *)c->uidx.p;
  a.nd0 = c->u_nd[0]; a.nd1 = c->u_nd[1]; a.nd2 = c->u_nd[2];
  a.ndp = gp.ndp;
  a.ulex = gp.ulex;
  a.nU = c->nU;
  a.nodes = d_nodes; a.n_nodes = n_nodes; a.node_stride = node_stride;
  a.n_max = gp.n_max; a.rmax = gp.rmax; a.boxcap = gp.boxcap; a.grid_limit = gp.grid;
  a.lex = gp.lex ? 1 : 0;
  a.dbg = c->tune.dbg;  // timing ablations, 0 in production
  a.l_pad = line_pad(c, a.l_nstride);
  a.l_zrows = skip;
  a.post = post_of(c, o);
  return a;
}

// `skip`: the state rows no kernel of this route stores to (GridArgs::l_zrows)
static int lists_grid(mplx_ctx *c, const GridPlan &gp, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                      const mplx_succ_lists *o, uint32_t skip) {
  if (int rc = ensure_tables(c)) return rc;
  if (int rc = ensure_blocked_bits(c)) return rc;
  // blocked bits patched by mplx_edit_map: the free-box shortcut is off until a launch of at least a few thousand
  // nodes makes its table (1.3 ms of scans at 512^3) worth rebuilding; a search's batches sample every node meanwhile
  if (c->sat_stale && n_nodes >= 4096)
    if (int rc = rebuild_sat(c)) return rc;
  mplx::GridArgs a = grid_args(c, gp, d_nodes, n_nodes, node_stride, o, skip);
  if (int rc = yaw_slot(c, &a.yaw)) return rc;
  if (int rc = prescreen(c, gp, &a)) return rc;
  arm_done(c, &a.done);
  const PairPlan pp = plan_pair(c, gp, a);
  if (int rc = pp.ok ? launch_pair(c, pp, a) : launch_grid(c, &a)) return rc;
  c->done_armed = a.done.flag != nullptr;
  if (a.yaw.amb) {
    mplx_ctx::YawPending p;
    p.kind = 0;
    p.g = a;
    p.g.live = nullptr;  // the fix pass walks its own node list
    p.g.live_n = nullptr;
    p.g.done = {};       // ... and is not the launch a caller waits for on the completion word
    c->yaw_pending.push_back(p);
  }
  c->last_route = MPLX_ROUTE_GRID;
  return MPLX_OK;
}

static int lists_tile(mplx_ctx *c, const TilePlan &tp, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                      const mplx_succ_lists *o) {
  if (int rc = ensure_tables(c)) return rc;
  mplx::TileArgs a = tile_args(c, tp, d_nodes, n_nodes, node_stride, o);
  arm_done(c, &a.done);
  HIP_TRY(c, mplx::launch_expand_tile(c->dim, c->prm.control, a, c->stream));
  c->done_armed = a.done.flag != nullptr;
  c->last_route = MPLX_ROUTE_TILE;
  return MPLX_OK;
}

// dense kernel into scratch, chunk by chunk, then ordered compaction on the device
static int lists_dense(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride, const mplx_succ_lists *o) {
  const int F = 4 * c->dim + 2;
  c->done_armed = false;
  const int64_t max_chunk_slots = (int64_t)(256u << 20) / (F * 8 + 21);  // ~256 MiB of scratch
  int64_t chunk_nodes = max_chunk_slots / c->nU;
  if (chunk_nodes < 1) chunk_nodes = 1;
  if (chunk_nodes > n_nodes) chunk_nodes = n_nodes;
  const int64_t cs = chunk_nodes * c->nU;
  if (int rc = ensure(c, c->d_status, (size_t)cs)) return rc;
  if (int rc = ensure(c, c->d_cost, (size_t)cs * 8)) return rc;
  if (int rc = ensure(c, c->d_hash, (size_t)cs * 8)) return rc;
  if (int rc = ensure(c, c->d_state, (size_t)cs * 8 * F)) return rc;
  if (int rc = ensure(c, c->d_iters, (size_t)cs * 4)) return rc;
  for (int64_t k0 = 0; k0 < n_nodes; k0 += chunk_nodes) {
    const int64_t nk = (n_nodes - k0) < chunk_nodes ? (n_nodes - k0) : chunk_nodes;
    mplx_succ d{};
    d.status = (uint8_t *)c->d_status.p;
    d.cost = (double *)c->d_cost.p;
    d.hash = (uint64_t *)c->d_hash.p;
    d.state = o->state ? (double *)c->d_state.p : nullptr;
    d.state_stride = cs;
    d.iters = o->iters ? (int32_t *)c->d_iters.p : nullptr;
    mplx::ExpandArgs a = expand_args(c, d_nodes + k0, nk, node_stride, &d);
    if (int rc = yaw_slot(c, &a.yaw)) return rc;
    HIP_TRY(c, mplx::launch_expand(c->dim, c->prm.control, a, c->stream));
    if (a.yaw.amb) {  // the scratch slots must be final before they are compacted: check this chunk now
      mplx_ctx::YawPending p;
      p.kind = 1;
      p.e = a;
      c->yaw_pending.push_back(p);
      if (int rc = resolve_pending(c)) return rc;
    }
    mplx::CompactArgs ca{};
    ca.status = d.status; ca.cost = d.cost; ca.hash = d.hash; ca.state = d.state; ca.iters = d.iters;
    ca.chunk_slots = cs; ca.nU = c->nU; ca.n_fields = F;
    ca.node_offset = k0; ca.n_nodes_chunk = nk;
    set_lists(c, o, &ca);
    HIP_TRY(c, mplx::launch_compact_lists(ca, c->stream));
  }
  if (o->heur || o->flags) {
    // the lane-per-pair kernel + compaction keeps no successor in registers at its list stores: the rows are made by
    // the stand-alone pass over the finished lists (post_kernel.hip; same values), which reads hash and state rows
    if (!o->hash || !o->state)
      return fail(c, MPLX_ERR_STATE, "heur / flags rows on the DENSE lists route need the hash and state rows as well");
    mplx::PostArgs pa{};
    pa.count = o->count;
    pa.hash = o->hash;
    pa.state = o->state;
    pa.sstride = o->state_stride;
    pa.n_nodes = n_nodes;
    pa.nstride = list_stride(c, o);
    for (int i = 0; i < F; i++) pa.goal[i] = c->goal_fuse.goal[i];
    pa.goal_hash = c->goal_fuse.goal_hash;
    pa.w = c->goal_fuse.w; pa.v_max = c->goal_fuse.v_max;
    pa.tol_pos = c->goal_fuse.tol_pos; pa.tol_vel = c->goal_fuse.tol_vel; pa.tol_acc = c->goal_fuse.tol_acc; pa.tol_yaw = c->goal_fuse.tol_yaw;
    pa.heur = o->heur;
    pa.flags = o->flags;
    HIP_TRY(c, mplx::launch_post_lists(c->dim, pa, c->stream));
  }
  c->last_route = MPLX_ROUTE_DENSE;
  return MPLX_OK;
}

// zero_rows (may be null = 0): in, the state rows of `o` the caller vouches hold +0.0 in every entry; out, the rows that
// still do after this launch (mplx_expand_lists_device_z, include/mplx.h).  Rows in both the caller's mask and
// const_zero_rows are not stored to by the kernels of the GRID route.  The yaw fix pass (resolve_pending) re-runs the
// same kernel with the same GridArgs -- it skips the same rows and only replaces entries of the others -- and
// mplx_pack_lists_device only reads: all-zero rows are invariant under both, so neither needs to know the mask.
int lists_device(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                 const mplx_succ_lists *o, uint32_t *zero_rows) {
  const int F = 4 * c->dim + 2;
  const int route = c->lists_route;
  const uint32_t const_rows = const_zero_rows(c->dim, c->prm.control);
  const uint32_t in_rows = zero_rows ? (*zero_rows & ((1u << F) - 1u)) : 0u;
  const uint32_t skip = o->state ? (in_rows & const_rows) : 0u;
  c->last_zero_rows = 0;
  // Until a route has launched with the skip, nothing is promised: a failure on the way, and the TILE and DENSE routes
  // (which store every row, the tile kernel from computed values), leave the caller with "no row is known to be zero".
  // Lists without state rows: no launch writes into them, the mask only narrows to the constant rows.
  if (zero_rows) *zero_rows = o->state ? 0u : (in_rows & const_rows);
  if ((o->heur || o->flags) && !c->has_goal)
    return fail(c, MPLX_ERR_STATE, "the heur / flags rows of the lists need a goal: call mplx_set_goal first");
  const GridPlan gp = (route == MPLX_ROUTE_AUTO || route == MPLX_ROUTE_GRID) ? plan_grid(c) : GridPlan();
  if (route == MPLX_ROUTE_GRID && !gp.ok)
    return fail(c, MPLX_ERR_STATE, "lists route GRID does not cover this configuration");
  bool grid = gp.ok;
  // A few hundred nodes with a large control table (the batches of a 3D search) are bound by the latency of
  // one node, and a node is a whole workgroup in the tiled kernel but a single wave in the factorised one:
  // 32 us against 54 us per launch for 16 - 256 nodes at |U| = 729 (profiles/micro/route_latency.py; no
  // difference for |U| <= 125).
  if (route == MPLX_ROUTE_AUTO && grid && n_nodes <= 512 && c->nU >= 512 && plan_tile(c).ok) grid = false;
  if (grid && n_nodes >= 0x7fffffffLL - 4096) grid = false;  // the factorised kernel counts nodes in 32 bits
  if (grid) {
    if (int rc = lists_grid(c, gp, d_nodes, n_nodes, node_stride, o, skip)) return rc;
    // every kernel of this route writes the literal +0.0 into the constant rows it does store to, and skipped `skip`
    c->last_zero_rows = skip;
    if (zero_rows && o->state) *zero_rows = skip;
    return MPLX_OK;
  }
  const TilePlan tp = (route == MPLX_ROUTE_AUTO || route == MPLX_ROUTE_TILE) ? plan_tile(c) : TilePlan();
  if (route == MPLX_ROUTE_TILE && !tp.ok)
    return fail(c, MPLX_ERR_STATE, "lists route TILE does not cover this configuration");
  if (tp.ok) return lists_tile(c, tp, d_nodes, n_nodes, node_stride, o);
  return lists_dense(c, d_nodes, n_nodes, node_stride, o);
}

// the checks and the launch behind mplx_expand_lists_device and _device_z (`fn`: the entry point, for the messages)
static int lists_entry(mplx_ctx *c, const char *fn, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                       const mplx_succ_lists *d_out, uint32_t *zero_rows) {
  if (!c) return MPLX_ERR_ARG;
  if (!d_out || !d_out->count || n_nodes < 0 || node_stride < n_nodes || (!d_nodes && n_nodes > 0))
    return fail(c, MPLX_ERR_ARG, "%s: bad arguments", fn);
  if (int rc = ctx_ready(c)) return rc;
  if (n_nodes == 0) return MPLX_OK;  // nothing is written: a mask stands as it is
  if (d_out->node_stride != 0 && d_out->node_stride < c->nU)
    return fail(c, MPLX_ERR_ARG, "%s: node_stride %lld < nU %d", fn, (long long)d_out->node_stride, c->nU);
  if (d_out->state && d_out->state_stride < n_nodes * list_stride(c, d_out))
    return fail(c, MPLX_ERR_ARG, "%s: state_stride < n_nodes*node_stride", fn);
  if (int rc = bind_device(c)) return rc;
  return lists_device(c, d_nodes, n_nodes, node_stride, d_out, zero_rows);
}

}  // namespace mplx_detail

using namespace mplx_detail;

extern "C" {

int mplx_expand_lists_device(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                             const mplx_succ_lists *d_out) {
  return lists_entry(c, "mplx_expand_lists_device", d_nodes, n_nodes, node_stride, d_out, nullptr);
}

int mplx_expand_lists_device_z(mplx_ctx *c, const double *d_nodes, int64_t n_nodes, int64_t node_stride,
                               const mplx_succ_lists *d_out, uint32_t *zero_rows) {
  if (!zero_rows || *zero_rows == 0) return mplx_expand_lists_device(c, d_nodes, n_nodes, node_stride, d_out);
  return lists_entry(c, "mplx_expand_lists_device_z", d_nodes, n_nodes, node_stride, d_out, zero_rows);
}

int mplx_lists_zero_fill(mplx_ctx *c, const mplx_succ_lists *d_lists, uint32_t *zero_rows) {
  if (!c) return MPLX_ERR_ARG;
  if (!d_lists || !zero_rows) return fail(c, MPLX_ERR_ARG, "mplx_lists_zero_fill: NULL argument");
  *zero_rows = 0;
  if (!d_lists->state) return MPLX_OK;
  if (d_lists->state_stride <= 0) return fail(c, MPLX_ERR_ARG, "mplx_lists_zero_fill: state_stride <= 0");
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // (a pending yaw fix pass would write after the fill)
  const int F = 4 * c->dim + 2;
  HIP_TRY(c, hipMemsetAsync(d_lists->state, 0, (size_t)F * (size_t)d_lists->state_stride * 8, c->stream));
  *zero_rows = (1u << F) - 1u;
  return MPLX_OK;
}

}  // extern "C"
