// mplx_poly.h -- the mplx_poly of include/mplx_solve.h as the sources that fill or read one see it (solve_api.cpp,
// limits_api.cpp): the segment table of its last solve or load, laid out for the K of that call (every array [row][K]),
// and the workspace of the elimination, which a limits call reuses for its per-segment maxima.
#ifndef MPLX_POLY_H
#define MPLX_POLY_H

#include "mplx_ctx.h"
#include "../../include/mplx_solve.h"

struct mplx_poly {
  mplx_ctx *c = nullptr;
  int64_t k_cap = 0;
  int32_t w_max = 0;
  mplx_detail::DevBuf mem;
  mplx_detail::DevBuf aux;  // scratch of mplx_shortcut when this poly is its pair set; grown on demand
  size_t o_S = 0, o_st = 0, o_T = 0, o_tau = 0, o_seg = 0, o_dt = 0, o_wp = 0, o_ws = 0;
  // the last solve or load
  int64_t n = 0;
  int32_t w = 0;  // its w_max
  int32_t control = 0;
  bool solved = false;
  // the Lambda of every problem (include/mplx_scale.h) and the scratch rows of the calls that build one; allocated on
  // first use for k_cap problems, indexed with the stride n of the last solve or load.  A solve or load drops it.
  mplx_detail::DevBuf lam;
  size_t l_n = 0, l_st = 0, l_seg = 0, l_Ts = 0, l_total = 0, l_pts = 0, l_npts = 0, l_scaled = 0, l_down = 0, l_res = 0;
  bool has_lambda = false;
  int32_t lam_mode = 0;  // MPLX_SCALE_REFERENCE / MPLX_SCALE_ROBUST of the call that built it
  mplx_detail::DevBuf conf;  // scratch of mplx_poly_conflicts (conflict_api.cpp); grown on demand
};

namespace mplx_detail {

// the table of the poly's last solve or load as the trajectory kernels take it
inline mplx::TrajArgs poly_table_args(mplx_poly *p) {
  const mplx_succ none{};
  mplx::TrajArgs a{};
  a.env = expand_args(p->c, nullptr, 0, 0, &none);
  char *base = (char *)p->mem.p;
  a.n_traj = p->n;
  a.horizon = p->w - 1;
  a.yaw = 1;
  a.poly = 1;
  a.tab_S = (int32_t *)(base + p->o_S);
  a.tab_n = nullptr;
  a.tab_status = (uint8_t *)(base + p->o_st);
  a.tab_T = (double *)(base + p->o_T);
  a.tab_tau = (double *)(base + p->o_tau);
  a.tab_seg = (double *)(base + p->o_seg);
  a.tab_dt = (const double *)(base + p->o_dt);
  a.tab_wp = (const double *)(base + p->o_wp);
  if (p->has_lambda) {
    char *lb = (char *)p->lam.p;
    a.lam = 1 + p->lam_mode;
    a.lam_n = (const int32_t *)(lb + p->l_n);
    a.lam_seg = (const double *)(lb + p->l_seg);
    a.lam_total = (const double *)(lb + p->l_total);
  }
  return a;
}

// scale_api.cpp: total_time[k] = the scaled total where problem k holds a Lambda (mplx_poly_info on a scaled set)
int poly_lambda_total(mplx_poly *p, double *d_total_time);

// reserve_poly_api.cpp: the launch of mplx_reserve_check_poly_device on table `a` (reserve_fill_args), device pointers,
// nothing validated: what the timed shortcut (limits_api.cpp) queues for its pair set
int reserve_check_poly_launch(const mplx::ReserveArgs &a, mplx_poly *p, const double *d_t_start, const double *d_radius,
                              double radius_all, const int32_t *d_ignore, int64_t *d_hit, uint8_t *d_status, int64_t *d_n_hit);

}  // namespace mplx_detail
#endif
