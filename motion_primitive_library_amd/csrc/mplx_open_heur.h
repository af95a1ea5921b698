// mplx_open_heur.h -- the heuristic of one node of an open set as a push computes it, for the re-key of
// include/mplx_anytime.h (open_rekey_kernel.hip), which reads the node's rows from the table where the push reads them
// from the frontier the table gathered.
//
// THIS IS A COPY of the heuristic body of open_push_kernel (open_kernel.hip, from `double s[4 * D + 1]` to the line that
// takes the larger of h and h_dyn), statement for statement, with the frontier's rows replaced by the table's.  It was
// meant to be the one text both kernels call; with the push calling it, 24 of the 36 open_push_kernel instantiations
// changed their SGPR count and four their VGPR count (DESIGN.md 4.28 has the table), so the push keeps its text and the
// figures it had.  Whoever changes one changes the other: tests/test_gpu_anytime.py holds the two to the same bits (a
// re-key at the eps of the pushes leaves every key as it was), for every mode below.  node_count and wave_min are the
// helpers of open_kernel.hip, copied for the same reason: that file is not touched.
#ifndef MPLX_OPEN_HEUR_H
#define MPLX_OPEN_HEUR_H

#include "mplx_internal.h"
#include "mplx_device_common.h"
#include "mplx_heur_math.h"

namespace mplx {
namespace {

constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;
constexpr uint8_t kIsOpen = 1, kIsGoal = 2, kSeen = 4;  // MPLX_OPEN_* of include/mplx_open.h

__device__ __forceinline__ int64_t node_count(const OpenArgs &A) {
  const int64_t n = A.t_ctl->n_nodes;
  return n < 0 ? 0 : (n < A.cap ? n : A.cap);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(v >> 32), d) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)v, d);
    v = o < v ? o : v;
  }
  return v;
}

// h and the tolerance bits of node `id` from the table's own rows, hash and query.  *q_out = the node's query.  False: the
// query column holds no query (never).
// MULTI: the goal is goals[query of the node] (mplx_open_set_goals), not the context's
// PRIOR: include/mplx_prior.h -- a query with a prior table takes its heuristic from where the prior is at the row's time
// (env_base.h:46-53)
// FIELD: include/mplx_field.h -- a query with a goal field takes max(Linf, res * (dist - 1)) where the default takes Linf,
// and +inf on a cell no chain leaves
// DYN: include/mplx_heur.h -- h = max(heur::robust, what the others give); a NaN (non-finite rows) stays
template <int D, bool MULTI, bool PRIOR, bool FIELD, bool DYN>
__device__ __forceinline__ bool open_heur(const OpenArgs &A, int64_t id, double *h_out, unsigned int *fl_out, int32_t *q_out) {
  const double *rows = A.t_state;  // [n_fields][cap]: what select's emit pass gathers a frontier from
  const int64_t stride = A.cap, r = id;
  double s[4 * D + 1];
#pragma unroll
  for (int i = 0; i < 3 * D; i++) s[i] = rows[(int64_t)i * stride + r];
  s[4 * D] = rows[(int64_t)(4 * D) * stride + r];
  const double t_row = PRIOR ? rows[(int64_t)(4 * D + 1) * stride + r] : 0.0;
  int32_t q = 0;
  if (MULTI && A.t_query) {
    q = A.t_query[id];
    if (q < 0 || q >= A.n_queries) return false;  // (never: the column holds only queries)
  }
  const PostFuse &GF = MULTI ? A.goals[q] : A.goal;
  MPLX_POST_GOAL(PG, GF, D)
  double h;
  unsigned int fl;
  dev::post_eval<D>(PG, A.t_hash[id], s, s + D, s + 2 * D, s[4 * D], &h, &fl);
  double h_dyn = 0.0;
  if (DYN && !(fl & 2u)) {  // (bit 1: the goal's own lattice state keeps h = 0, env_base.h:47)
    const int32_t *ctl = (MULTI && A.dyn_controls) ? A.dyn_controls + 2 * (int64_t)q : A.dyn_control;
    h_dyn = heur::robust<D>(s, PG.g, ctl[0], ctl[1], PG.w, PG.v_max);
  }
  if (PRIOR && !(fl & 2u)) {  // (bit 1: the goal's own lattice state keeps h = 0, env_base.h:47)
    const int32_t ns = A.prior_n[q];
    const double x = t_row > 0 ? t_row / A.prior_dt : 0.0;  // env_base.h:48
    if (ns > 0 && x < (double)ns) {
      int64_t k = (int64_t)x;
      k = k < 0 ? 0 : (k < A.prior_cap ? k : A.prior_cap - 1);  // (0 <= x < ns <= prior_cap: never moves)
      const double *pp = A.prior_pos + ((int64_t)q * A.prior_cap + k) * D;
      double m = 0;
#pragma unroll
      for (int i = 0; i < D; i++) {
        const double d = fabs(s[i] - pp[i]);
        m = d > m ? d : m;
      }
      const double lin = PG.v_max > 0 ? PG.w * m / PG.v_max : PG.w * m;
      h = lin + A.prior_togo[(int64_t)q * A.prior_cap + k];
    }
  }
  if (FIELD && !(fl & 2u)) {  // (bit 1: the goal's own lattice state keeps h = 0)
    const int32_t fq = A.field_of_query[q];
    if (fq >= 0 && fq < A.field_F) {  // (the host checked the entries: never out of range)
      bool inside = true;
      int64_t idx = 0, mul = 1;
#pragma unroll
      for (int i = 0; i < D; i++) {
        const double c = round((s[i] - A.field_org[i]) / A.field_res - 0.5);  // map_util.h:103-108
        const bool in = c >= 0.0 && c < (double)A.field_dim[i];  // compared as a double: NaN and huge values are outside
        inside = inside && in;
        idx += (in ? (int64_t)c : 0) * mul;
        mul *= A.field_dim[i];
      }
      const int32_t n = inside ? A.field_dist[(int64_t)fq * A.field_cells + idx] : -1;
      if (n < 0) {
        h = __longlong_as_double((long long)kInfBits);
      } else {
        double L = 0;  // post_eval's lpNorm<Infinity> of pos - goal.pos
#pragma unroll
        for (int i = 0; i < D; i++) {
          const double d = fabs(s[i] - PG.g[i]);
          L = d > L ? d : L;
        }
        const double G = A.field_res * (double)(n - 1 > 0 ? n - 1 : 0);
        if (G > L) h = PG.v_max > 0 ? PG.w * G / PG.v_max : PG.w * G;  // (G <= L: post_eval's h, bit for bit)
      }
    }
  }
  if (DYN && !(h_dyn <= h)) h = h_dyn;  // the larger; a NaN stays
  *h_out = h;
  *fl_out = fl;
  *q_out = q;
  return true;
}

}  // namespace
}  // namespace mplx
#endif
