// limits_api.cpp -- C ABI of include/mplx_limits.h: caller-given segments into an mplx_poly (poly_load_kernel) and the
// dynamic limits of the set a poly holds (poly_limits_kernel), both in limits_kernel.hip.  The host-pointer twins stage
// through the context's arena and scatter the compact device rows into the caller's strides, as solve_api.cpp does.
// The timed shortcut of include/mplx_reserve_poly.h is the shortcut with a reservation table, and stands next to it.
#include "mplx_poly.h"
#include "../../include/mplx_limits.h"
#include "../../include/mplx_reserve_poly.h"

using namespace mplx_detail;

namespace {

int check_load(mplx_poly *p, const char *who, const mplx_poly_load_in *in, const mplx_poly_load_out *out) {
  mplx_ctx *c = p->c;
  if (!in || !out || in->n_prob < 0 || in->w_max < 2 || in->w_max > p->w_max || in->n_prob > p->k_cap)
    return fail(c, MPLX_ERR_ARG, "%s: NULL in / out, w_max outside [2, %d] or more than %lld problems", who, p->w_max, (long long)p->k_cap);
  const int ctl = in->control & 0x0f;
  if ((in->control & ~0x1f) || (ctl != MPLX_VEL && ctl != MPLX_ACC && ctl != MPLX_JRK && ctl != MPLX_SNP))
    return fail(c, MPLX_ERR_ARG, "%s: control must be VEL, ACC, JRK or SNP (with or without the yaw bit)", who);
  const int64_t K = in->n_prob;
  if (in->src || in->src_index) {  // the gather form
    if (!in->src || !in->src_index || in->src == p || in->src->c != c || !in->src->solved || in->index_stride < K)
      return fail(c, MPLX_ERR_ARG, "%s: the gather form needs src (a filled poly of this context, not the target) and src_index with a stride >= n_prob", who);
    if (out->taus && out->taus_stride < K) return fail(c, MPLX_ERR_ARG, "%s: a stride is smaller than n_prob", who);
    return MPLX_OK;
  }
  if (K > 0 && (!in->coeff || !in->dts)) return fail(c, MPLX_ERR_ARG, "%s: NULL coeff or dts", who);
  if (in->dt_stride < K || in->coeff_stride < K || (out->taus && out->taus_stride < K))
    return fail(c, MPLX_ERR_ARG, "%s: a stride is smaller than n_prob", who);
  return MPLX_OK;
}

int load_launch(mplx_poly *p, const mplx_poly_load_in *in, const mplx_poly_load_out *out) {
  mplx_ctx *c = p->c;
  p->n = in->n_prob;
  p->w = in->w_max;
  p->solved = true;
  p->control = in->control;
  p->has_lambda = false;  // a load clears the Lambda, and the gather form does not copy the source's (include/mplx_scale.h)
  const mplx::TrajArgs t = poly_table_args(p);
  mplx::PolyLoadArgs a{};
  a.n_prob = in->n_prob;
  a.w_max = in->w_max;
  a.n_segs = in->n_segs;
  a.dts = in->dts; a.dt_stride = in->dt_stride;
  a.coeff = in->coeff; a.coeff_stride = in->coeff_stride;
  if (in->src_index) {
    const mplx::TrajArgs st = poly_table_args(in->src);
    a.src_index = in->src_index; a.index_stride = in->index_stride; a.src_n = in->src->n;
    a.src_S = st.tab_S; a.src_seg = st.tab_seg; a.src_dt = st.tab_dt;
  }
  a.tab_S = t.tab_S; a.tab_status = t.tab_status; a.tab_T = t.tab_T; a.tab_tau = t.tab_tau; a.tab_seg = t.tab_seg;
  a.tab_dt = (double *)t.tab_dt; a.tab_wp = (double *)t.tab_wp;
  a.status = out->status; a.n_segs_out = out->n_segs; a.total_time = out->total_time;
  a.taus_out = out->taus; a.taus_stride = out->taus_stride;
  HIP_TRY(c, mplx::launch_poly_load(c->dim, a, c->stream));
  return MPLX_OK;
}

int check_limits(mplx_poly *p, const char *who, const mplx_limits_in *in, const mplx_limits_out *out) {
  mplx_ctx *c = p->c;
  if (!in || !out) return fail(c, MPLX_ERR_ARG, "%s: NULL in / out", who);
  if (in->mode != MPLX_LIMITS_REFERENCE && in->mode != MPLX_LIMITS_ALL_ROOTS)
    return fail(c, MPLX_ERR_ARG, "%s: mode must be MPLX_LIMITS_REFERENCE or MPLX_LIMITS_ALL_ROOTS", who);
  if (!p->solved) return fail(c, MPLX_ERR_STATE, "%s: nothing has been solved or loaded into this poly", who);
  if ((out->max_vel || out->max_acc || out->max_jrk) && out->max_stride < p->n)
    return fail(c, MPLX_ERR_ARG, "%s: max_stride < n_prob", who);
  return MPLX_OK;
}

int limits_launch(mplx_poly *p, const mplx_limits_in *in, const mplx_limits_out *o) {
  mplx_ctx *c = p->c;
  const mplx::TrajArgs t = poly_table_args(p);
  mplx::LimitsArgs a{};
  a.n_prob = p->n;
  a.s_max = p->w - 1;
  a.control = p->control;
  a.all_roots = in->mode == MPLX_LIMITS_ALL_ROOTS;
  a.mv = in->mv; a.ma = in->ma; a.mj = in->mj;
  a.tab_S = t.tab_S; a.tab_seg = t.tab_seg; a.tab_dt = t.tab_dt;
  a.seg_max = (double *)((char *)p->mem.p + p->o_ws);  // (w - 1) * 3 D rows of the w_max * (9 + 3 D) there are
  a.max_vel = o->max_vel; a.max_acc = o->max_acc; a.max_jrk = o->max_jrk; a.max_stride = o->max_stride;
  a.exceed = o->exceed; a.valid = o->valid; a.first_bad = o->first_bad;
  HIP_TRY(c, mplx::launch_poly_limits(c->dim, a, c->stream));
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_poly_load_device(mplx_poly *p, const mplx_poly_load_in *d_in, const mplx_poly_load_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_load(p, "mplx_poly_load_device", d_in, d_out)) return rc;
  if (d_in->n_prob == 0) return MPLX_OK;
  if (int rc = bind_device(p->c)) return rc;
  return load_launch(p, d_in, d_out);
}

int mplx_poly_load(mplx_poly *p, const mplx_poly_load_in *h_in, const mplx_poly_load_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_load(p, "mplx_poly_load", h_in, h_out)) return rc;
  if (h_in->n_prob == 0) return MPLX_OK;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // the arena is shared with the other host-pointer calls
  const size_t n = (size_t)h_in->n_prob, W = (size_t)h_in->w_max, D = (size_t)c->dim, cr = (W - 1) * (D + 1) * 6;
  const bool gather = h_in->src_index != nullptr;  // (the gather form stages no input: src_index is device memory)
  StageRows s;
  const auto i_S = s.in(gather ? nullptr : h_in->n_segs, n * 4), i_dts = s.in_rows(gather ? nullptr : h_in->dts, (size_t)h_in->dt_stride * 8, n * 8, W - 1),
             i_c = s.in_rows(gather ? nullptr : h_in->coeff, (size_t)h_in->coeff_stride * 8, n * 8, cr);
  const auto o_st = s.landed(n), o_T = s.landed(n * 8), o_t = s.landed(h_out->taus, W * n * 8),
             t_S = s.landed_from((char *)p->mem.p + p->o_S, n * 4);  // (S_k is read from the poly's table: 0 for a failed problem)
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_poly_load_in in = *h_in;
  if (!gather) {
    in.n_segs = s.dev<int32_t>(i_S);
    in.dts = s.dev<double>(i_dts); in.dt_stride = (int64_t)n;
    in.coeff = s.dev<double>(i_c); in.coeff_stride = (int64_t)n;
  }
  mplx_poly_load_out o{};
  o.status = s.dev<uint8_t>(o_st);
  o.total_time = s.dev<double>(o_T);
  o.taus = s.dev<double>(o_t); o.taus_stride = (int64_t)n;
  if (int rc = load_launch(p, &in, &o)) return rc;
  if (int rc = stage_fetch(c, &s)) return rc;
  const uint8_t *st = s.host<uint8_t>(o_st);
  const int32_t *S = s.host<int32_t>(t_S);
  const double *T = s.host<double>(o_T), *ta = s.host<double>(o_t);
  for (size_t k = 0; k < n; k++) {
    if (h_out->status) h_out->status[k] = st[k];
    const size_t Sk = (size_t)S[k];
    if (Sk == 0) continue;  // a failed problem: its status only
    if (h_out->n_segs) h_out->n_segs[k] = S[k];
    if (h_out->total_time) h_out->total_time[k] = T[k];
    for (size_t r = 0; r <= Sk && h_out->taus; r++) h_out->taus[(int64_t)r * h_out->taus_stride + (int64_t)k] = ta[r * n + k];
  }
  return MPLX_OK;
}

int mplx_poly_limits_device(mplx_poly *p, const mplx_limits_in *in, const mplx_limits_out *d_out) {
  if (!p) return MPLX_ERR_ARG;
  if (int rc = check_limits(p, "mplx_poly_limits_device", in, d_out)) return rc;
  if (int rc = bind_device(p->c)) return rc;
  return limits_launch(p, in, d_out);
}

int mplx_poly_limits(mplx_poly *p, const mplx_limits_in *in, const mplx_limits_out *h_out) {
  if (!p) return MPLX_ERR_ARG;
  mplx_ctx *c = p->c;
  if (int rc = check_limits(p, "mplx_poly_limits", in, h_out)) return rc;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t n = (size_t)p->n, D = (size_t)c->dim;
  double *const h_max[3] = {h_out->max_vel, h_out->max_acc, h_out->max_jrk};
  StageRows s;
  const StageRows::Row o_m[3] = {s.landed(h_max[0], D * n * 8), s.landed(h_max[1], D * n * 8), s.landed(h_max[2], D * n * 8)};
  const auto o_e = s.landed(h_out->exceed, n), o_v = s.landed(h_out->valid, n), o_f = s.landed(h_out->first_bad, n * 4),
             t_S = s.landed_from((char *)p->mem.p + p->o_S, n * 4);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_limits_out o{};
  o.max_vel = s.dev<double>(o_m[0]); o.max_acc = s.dev<double>(o_m[1]); o.max_jrk = s.dev<double>(o_m[2]);
  o.max_stride = (int64_t)n;
  o.exceed = s.dev<uint8_t>(o_e); o.valid = s.dev<uint8_t>(o_v); o.first_bad = s.dev<int32_t>(o_f);
  if (int rc = limits_launch(p, in, &o)) return rc;
  if (int rc = stage_fetch(c, &s)) return rc;
  const int32_t *S = s.host<int32_t>(t_S), *fb = s.host<int32_t>(o_f);
  const uint8_t *ex = s.host<uint8_t>(o_e), *va = s.host<uint8_t>(o_v);
  const double *const mx[3] = {s.host<double>(o_m[0]), s.host<double>(o_m[1]), s.host<double>(o_m[2])};
  for (size_t k = 0; k < n; k++) {
    if (S[k] == 0) continue;  // a failed problem keeps the caller's bytes
    for (int q = 0; q < 3; q++)
      for (size_t i = 0; i < D && h_max[q]; i++) h_max[q][(int64_t)i * h_out->max_stride + (int64_t)k] = mx[q][i * n + k];
    if (h_out->exceed) h_out->exceed[k] = ex[k];
    if (h_out->valid) h_out->valid[k] = va[k];
    if (h_out->first_bad) h_out->first_bad[k] = fb[k];
  }
  return MPLX_OK;
}

}  // extern "C"

namespace {

int check_shortcut(mplx_poly *pairs, mplx_poly *res, const char *who, const mplx_shortcut_in *in, const mplx_shortcut_out *out, int64_t *np) {
  mplx_ctx *c = pairs->c;
  if (!res || !in || !out || res == pairs || res->c != c) return fail(c, MPLX_ERR_ARG, "%s: NULL or equal polys, polys of two contexts, NULL in / out", who);
  const int ctl = in->control & 0x0f;
  if ((in->control & ~0x1f) || (ctl != MPLX_VEL && ctl != MPLX_ACC && ctl != MPLX_JRK))
    return fail(c, MPLX_ERR_ARG, "%s: control must be VEL, ACC or JRK (with or without the yaw bit)", who);
  if (in->n_query < 0 || in->w_max < 2 || in->max_hop < 1 || in->w_max > res->w_max || in->n_query > res->k_cap)
    return fail(c, MPLX_ERR_ARG, "%s: n_query < 0, w_max < 2, max_hop < 1, or a result poly smaller than Q x w_max", who);
  const double npd = (double)in->n_query * (double)(in->w_max - 1) * (double)in->max_hop;
  if (npd > (double)pairs->k_cap || npd > 2147483647.0)
    return fail(c, MPLX_ERR_ARG, "%s: the pair poly holds fewer than Q (w_max - 1) max_hop problems", who);
  *np = in->n_query * (in->w_max - 1) * in->max_hop;
  if (in->n_query > 0 && !in->states) return fail(c, MPLX_ERR_ARG, "%s: NULL states", who);
  if (in->stride < in->n_query || (out->keep && out->keep_stride < in->n_query)) return fail(c, MPLX_ERR_ARG, "%s: a stride is smaller than n_query", who);
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "%s: set the map first", who);
  if (!(c->prm.v_max > 0)) return fail(c, MPLX_ERR_STATE, "%s: v_max must be > 0 (env_map.h:231)", who);
  return MPLX_OK;
}

// the reservation table of a timed shortcut: NULL res / another context / a number of queries other than n_query:
// MPLX_ERR_ARG; before a fill or mplx_reserve_set_queries: MPLX_ERR_STATE
int check_table(mplx_poly *pairs, const char *who, const mplx_shortcut_in *in, mplx_reserve *table, mplx::ReserveArgs *t) {
  mplx_ctx *c = pairs->c;
  if (!table) return fail(c, MPLX_ERR_ARG, "%s: NULL reservation table", who);
  mplx_ctx *tc = nullptr;
  const int rc = reserve_table_args(table, who, &tc, t);  // (sets tc whatever it answers)
  if (tc != c) return fail(c, MPLX_ERR_ARG, "%s: the reservation table belongs to another context", who);
  if (rc) return rc;
  if (t->Q != in->n_query)
    return fail(c, MPLX_ERR_ARG, "%s: %d queries were set, the shortcut has %lld", who, (int)t->Q, (long long)in->n_query);
  return MPLX_OK;
}

// everything queued on the stream, no read-back: pairs -> solve -> info, limits, traverse -> costs, programme -> gather.
// table (optional): after the solve the rows of the pair set and its check against the table (include/mplx_reserve_poly.h);
// without it exactly the launches of mplx_shortcut_device.
int shortcut_launch(mplx_poly *pairs, mplx_poly *res, const mplx_shortcut_in *in, const mplx_shortcut_out *out, int64_t NP,
                    const mplx::ReserveArgs *table = nullptr, int64_t *d_chain_hit = nullptr) {
  mplx_ctx *c = pairs->c;
  const size_t P = (size_t)NP, Q = (size_t)in->n_query, W = (size_t)in->w_max, F = 4 * (size_t)c->dim + 2;
  StageLayout l;  // (only the carving)
  const size_t o_wp = l.add(F * 2 * P * 8), o_dt = l.add(P * 8), o_eff = l.add(5 * P * 8), o_trav = l.add(P * 8), o_ec = l.add(P * 8),
               o_dist = l.add(W * Q * 8), o_nwp = l.add(P * 4), o_pred = l.add(W * Q * 4), o_src = l.add((W - 1) * Q * 4),
               o_fl = l.add(2 * P), o_valid = l.add(P), o_st = l.add(P);
  const size_t o_ts = l.add(table ? P * 8 : 0), o_rad = l.add(table ? P * 8 : 0), o_ign = l.add(table ? P * 4 : 0),
               o_hit = l.add(table ? P * 8 : 0);
  if (int rc = ensure(c, pairs->aux, l.total)) return rc;
  char *b = (char *)pairs->aux.p;
  mplx::ShortcutArgs a{};
  a.n_query = in->n_query; a.w_max = in->w_max; a.max_hop = in->max_hop; a.order = control_order(in->control);
  a.w = c->prm.w;
  a.states = in->states; a.stride = in->stride; a.n_wp = in->n_wp;
  a.pair_wp = (double *)(b + o_wp); a.pair_dt = (double *)(b + o_dt); a.pair_nwp = (int32_t *)(b + o_nwp); a.pair_flags = (uint8_t *)(b + o_fl);
  a.pair_status = (uint8_t *)(b + o_st); a.pair_valid = (uint8_t *)(b + o_valid);
  a.pair_effort = (double *)(b + o_eff); a.pair_trav = (double *)(b + o_trav);
  a.dist = (double *)(b + o_dist); a.pred = (int32_t *)(b + o_pred); a.src_index = (int32_t *)(b + o_src);
  a.status = out->status; a.n_keep = out->n_keep; a.keep = out->keep; a.keep_stride = out->keep_stride;
  a.cost = out->cost; a.chain_cost = out->chain_cost;
  a.edge_cost = out->edge_cost ? out->edge_cost : (double *)(b + o_ec);
  HIP_TRY(c, mplx::launch_shortcut_pairs(c->dim, a, c->stream));
  mplx_solve_in si{};
  si.waypoints = a.pair_wp; si.n_prob = NP; si.w_max = 2; si.wp_stride = NP; si.n_wp = a.pair_nwp;
  si.dts = a.pair_dt; si.dt_stride = NP; si.v = 1.0; si.control = in->control; si.yaw_control = MPLX_VEL;
  si.wp_flags = a.pair_flags; si.flag_stride = NP;
  mplx_solve_out so = out->pair_out ? *out->pair_out : mplx_solve_out{};
  uint8_t *caller_status = so.status;
  so.status = (uint8_t *)a.pair_status;
  if (int rc = mplx_solve_device(pairs, &si, &so)) return rc;
  if (caller_status) HIP_TRY(c, hipMemcpyAsync(caller_status, a.pair_status, P, hipMemcpyDeviceToDevice, c->stream));
  a.pair_T = (const double *)((char *)pairs->mem.p + pairs->o_T);
  if (table) {
    mplx::PairRowsArgs ra{};
    ra.n_query = in->n_query; ra.w_max = in->w_max; ra.max_hop = in->max_hop;
    ra.t_row = in->states + (int64_t)(F - 1) * in->w_max * in->stride; ra.stride = in->stride;
    ra.q_t0 = table->q_t0; ra.q_r = table->q_r; ra.q_ignore = table->q_ignore;
    ra.t_start = (double *)(b + o_ts); ra.radius = (double *)(b + o_rad); ra.ignore = (int32_t *)(b + o_ign);
    HIP_TRY(c, mplx::launch_reserve_pair_rows(ra, c->stream));
    if (int rc = reserve_check_poly_launch(*table, pairs, ra.t_start, ra.radius, 0.0, ra.ignore, (int64_t *)(b + o_hit), nullptr, nullptr))
      return rc;
    a.pair_hit = (const long long *)(b + o_hit);
    a.chain_hit = (long long *)d_chain_hit;
  }
  mplx_traj_info_out io{};
  io.effort = (double *)a.pair_effort; io.effort_stride = NP;
  if (int rc = mplx_poly_info_device(pairs, &io)) return rc;
  HIP_TRY(c, hipMemsetAsync((void *)a.pair_valid, 0, P, c->stream));  // (the limits skip a failed pair)
  mplx_limits_in li{c->prm.v_max, c->prm.a_max, c->prm.j_max, MPLX_LIMITS_ALL_ROOTS};
  mplx_limits_out lo{};
  lo.valid = (uint8_t *)a.pair_valid;
  if (int rc = mplx_poly_limits_device(pairs, &li, &lo)) return rc;
  mplx_traj_traverse_out to{};
  to.cost = (double *)a.pair_trav;
  if (int rc = mplx_poly_traverse_device(pairs, 0, &to)) return rc;
  HIP_TRY(c, mplx::launch_shortcut_dp(a, c->stream));
  mplx_poly_load_in gi{};
  gi.n_prob = in->n_query; gi.w_max = in->w_max; gi.control = in->control;
  gi.src = pairs; gi.src_index = a.src_index; gi.index_stride = in->n_query;
  mplx_poly_load_out go{};
  return mplx_poly_load_device(res, &gi, &go);
}

// mplx_shortcut / mplx_shortcut_timed on host rows: they differ in the table and the chain_hit row it adds, and in
// nothing else.  The calls inside stage nothing: they are device forms (rule 4 of the arena).
int shortcut_host(mplx_poly *pairs, mplx_poly *res, const mplx_shortcut_in *h_in, const mplx_shortcut_out *h_out, int64_t NP,
                  const mplx::ReserveArgs *table, int64_t *h_chain_hit) {
  mplx_ctx *c = pairs->c;
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const size_t Q = (size_t)h_in->n_query, W = (size_t)h_in->w_max, F = 4 * (size_t)c->dim + 2, P = (size_t)NP;
  StageRows s;
  const auto i_st = s.in_rows(h_in->states, (size_t)h_in->stride * 8, Q * 8, F * W), i_n = s.in(h_in->n_wp, Q * 4);
  const auto o_s = s.out_or_scratch(h_out->status, Q), o_nk = s.out_or_scratch(h_out->n_keep, Q * 4),
             o_k = s.landed_or_scratch(h_out->keep, W * Q * 4), o_c = s.out_or_scratch(h_out->cost, Q * 8),
             o_cc = s.out_or_scratch(h_out->chain_cost, Q * 8), o_e = s.out_or_scratch(h_out->edge_cost, P * 8),
             o_ch = s.out(table ? h_chain_hit : nullptr, Q * 8);
  if (int rc = stage_commit(c, &s)) return rc;
  mplx_shortcut_in in = *h_in;
  in.states = s.dev<double>(i_st); in.stride = (int64_t)Q;
  in.n_wp = s.dev<int32_t>(i_n);
  mplx_shortcut_out o{};
  o.status = s.dev<uint8_t>(o_s); o.n_keep = s.dev<int32_t>(o_nk); o.keep = s.dev<int32_t>(o_k); o.keep_stride = (int64_t)Q;
  o.cost = s.dev<double>(o_c); o.chain_cost = s.dev<double>(o_cc); o.edge_cost = s.dev<double>(o_e);
  if (int rc = shortcut_launch(pairs, res, &in, &o, NP, table, s.dev<int64_t>(o_ch))) return rc;
  if (int rc = stage_fetch(c, &s)) return rc;
  const int32_t *keep = s.host<int32_t>(o_k);
  for (size_t w = 0; w < W && keep; w++)
    for (size_t k = 0; k < Q; k++) h_out->keep[(int64_t)w * h_out->keep_stride + (int64_t)k] = keep[w * Q + k];
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_shortcut_device(mplx_poly *pairs, mplx_poly *res, const mplx_shortcut_in *d_in, const mplx_shortcut_out *d_out) {
  if (!pairs) return MPLX_ERR_ARG;
  int64_t NP = 0;
  if (int rc = check_shortcut(pairs, res, "mplx_shortcut_device", d_in, d_out, &NP)) return rc;
  if (NP == 0) return MPLX_OK;
  if (int rc = bind_device(pairs->c)) return rc;
  return shortcut_launch(pairs, res, d_in, d_out, NP);
}

int mplx_shortcut(mplx_poly *pairs, mplx_poly *res, const mplx_shortcut_in *h_in, const mplx_shortcut_out *h_out) {
  if (!pairs) return MPLX_ERR_ARG;
  mplx_ctx *c = pairs->c;
  int64_t NP = 0;
  if (int rc = check_shortcut(pairs, res, "mplx_shortcut", h_in, h_out, &NP)) return rc;
  if (h_out->pair_out) return fail(c, MPLX_ERR_ARG, "mplx_shortcut: pair_out is for the _device form");
  if (NP == 0) return MPLX_OK;
  return shortcut_host(pairs, res, h_in, h_out, NP, nullptr, nullptr);
}

int mplx_shortcut_timed_device(mplx_poly *pairs, mplx_poly *res, const mplx_shortcut_in *d_in, const mplx_shortcut_out *d_out,
                               mplx_reserve *table, int64_t *d_chain_hit) {
  if (!pairs) return MPLX_ERR_ARG;
  const char *who = "mplx_shortcut_timed_device";
  int64_t NP = 0;
  if (int rc = check_shortcut(pairs, res, who, d_in, d_out, &NP)) return rc;
  mplx::ReserveArgs t{};
  if (int rc = check_table(pairs, who, d_in, table, &t)) return rc;
  if (NP == 0) return MPLX_OK;
  if (int rc = bind_device(pairs->c)) return rc;
  return shortcut_launch(pairs, res, d_in, d_out, NP, &t, d_chain_hit);
}

int mplx_shortcut_timed(mplx_poly *pairs, mplx_poly *res, const mplx_shortcut_in *h_in, const mplx_shortcut_out *h_out,
                        mplx_reserve *table, int64_t *h_chain_hit) {
  if (!pairs) return MPLX_ERR_ARG;
  mplx_ctx *c = pairs->c;
  const char *who = "mplx_shortcut_timed";
  int64_t NP = 0;
  if (int rc = check_shortcut(pairs, res, who, h_in, h_out, &NP)) return rc;
  if (h_out->pair_out) return fail(c, MPLX_ERR_ARG, "%s: pair_out is for the _device form", who);
  mplx::ReserveArgs t{};
  if (int rc = check_table(pairs, who, h_in, table, &t)) return rc;
  if (NP == 0) return MPLX_OK;
  return shortcut_host(pairs, res, h_in, h_out, NP, &t, h_chain_hit);
}

}  // extern "C"
