// open_rekey_kernel.hip -- the re-key of an open set and the lower bound of its open nodes (include/mplx_anytime.h): what
// ARA* does to its queue when eps falls (every key becomes g + eps * h again) and what it reports (min over open of g + h),
// for all nodes of a table at once.
//
// The discipline of open_kernel.hip holds: a launch boundary is the only ordering, no workgroup waits for another, only
// order-free atomics decide anything (a 64-bit atomicMin on the bit patterns of non-negative doubles, atomicAdd on counts),
// every id and query is checked where it is formed, every output is a pure function of the inputs.  A table with a status
// bit makes every launch return at its first instruction.
//
// Three launches:
//   reset    one lane per query: its control block (lower = +inf, the counts 0)
//   re-key   one lane per node id: h as a push computes it (mplx_open_heur.h) from the table's rows, L = g + h,
//            f = g + eps * h; per (wave, query) one atomicMin and three atomicAdds
//   finish   one lane per query: the bound, to the caller's device memory and to the pinned mirror
#include "mplx_open_heur.h"

namespace mplx {
namespace {

constexpr int kBlock = 256;

template <int D, bool MULTI, bool PRIOR, bool FIELD, bool DYN>
__global__ __launch_bounds__(kBlock) void open_rekey_kernel(const RekeyArgs R) {
  const OpenArgs &A = R.o;
  if (A.t_ctl->status) return;  // (uniform)
  const int64_t id = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  bool seen = false, open = false, pruned = false, rekeyed = false;
  int32_t q = 0;
  unsigned long long lb = kInfBits;
  if (id < node_count(A)) {
    const uint8_t flg = A.flags[id];
    double h;
    unsigned int fl;
    if ((flg & kSeen) && open_heur<D, MULTI, PRIOR, FIELD, DYN>(A, id, &h, &fl, &q)) {  // (q is within [0, n_queries))
      seen = true;
      open = (flg & kIsOpen) != 0;
      const double g = __longlong_as_double((long long)A.t_g[id]);
      const double L = g + h;
      if (open && L >= 0.0) lb = (unsigned long long)__double_as_longlong(L + 0.0);  // (a NaN bounds nothing)
      if (R.write) {
        double f = g;
        if (A.eps != 0.0) {
          const double eh = A.eps * h;
          f = g + eh;
        }
        if (f >= 0.0) {
          f = f + 0.0;  // -0.0 -> +0.0, as the push
          A.f[id] = (unsigned long long)__double_as_longlong(f);
          rekeyed = true;
        }
        if (R.cut && open) {
          const double cq = R.cut[q];
          if (cq < __longlong_as_double((long long)kInfBits) && L >= cq) {  // (+inf prunes nothing; a tie is pruned)
            A.flags[id] = (uint8_t)(flg & ~kIsOpen);
            pruned = true;
          }
        }
      }
    }
  }
  unsigned long long left = __ballot(seen);  // the lanes with something to say
  while (left) {  // one round per distinct query present, at most 64 (one, when the wave holds one query)
    const int32_t qq = __shfl(q, __builtin_ctzll(left));
    const bool mine = seen && q == qq;
    const unsigned long long bm = __ballot(mine), bo = __ballot(mine && open), bp = __ballot(mine && pruned), br = __ballot(mine && rekeyed);
    unsigned long long v = (mine && open) ? lb : kInfBits;
    if (bo) v = wave_min(v);
    if ((threadIdx.x & 63) == 0) {
      RekeyCtl *c = R.rctl + qq;
      if (bo) {
        atomicMin(&c->lower_bits, v);
        atomicAdd(&c->n_open, (unsigned long long)__popcll(bo));
      }
      if (bp) atomicAdd(&c->n_pruned, (unsigned long long)__popcll(bp));
      if (br) atomicAdd(&c->n_rekeyed, (unsigned long long)__popcll(br));
    }
    left &= ~bm;
  }
}

__global__ __launch_bounds__(kBlock) void open_rekey_reset_kernel(const RekeyArgs R) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= R.o.n_queries) return;
  RekeyCtl *c = R.rctl + q;
  c->lower_bits = kInfBits;
  c->n_open = 0;
  c->n_pruned = 0;
  c->n_rekeyed = 0;
}

__global__ __launch_bounds__(kBlock) void open_rekey_finish_kernel(const RekeyArgs R) {
  if (R.o.t_ctl->status) return;
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= R.o.n_queries) return;
  const RekeyCtl *c = R.rctl + q;
  OpenBound B;
  B.lower = __longlong_as_double((long long)c->lower_bits);
  B.n_open = (int64_t)c->n_open;
  B.n_pruned = (int64_t)c->n_pruned;
  B.n_rekeyed = (int64_t)c->n_rekeyed;
  if (R.d_bound) R.d_bound[q] = B;
  OpenBound *m = R.mirror + q;  // pinned: what the host reads, without a copy, once it has waited for the stream
  __hip_atomic_store(&m->lower, B.lower, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->n_open, B.n_open, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->n_pruned, B.n_pruned, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&m->n_rekeyed, B.n_rekeyed, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int D, bool MULTI, bool PRIOR = false, bool FIELD = false, bool DYN = false>
void rekey(dim3 grid, dim3 block, hipStream_t s, const RekeyArgs &r) {
  hipLaunchKernelGGL((open_rekey_kernel<D, MULTI, PRIOR, FIELD, DYN>), grid, block, 0, s, r);
}

template <int D>
void rekey_dim(dim3 grid, dim3 block, hipStream_t s, const RekeyArgs &r) {
  const OpenArgs &a = r.o;
  if (a.dyn) {
    if (a.field_dist) {
      if (a.goals) rekey<D, true, false, true, true>(grid, block, s, r);
      else rekey<D, false, false, true, true>(grid, block, s, r);
    } else {
      if (a.goals) rekey<D, true, false, false, true>(grid, block, s, r);
      else rekey<D, false, false, false, true>(grid, block, s, r);
    }
  } else if (a.field_dist) {
    if (a.goals) rekey<D, true, false, true>(grid, block, s, r);
    else rekey<D, false, false, true>(grid, block, s, r);
  } else if (a.prior_n) {
    rekey<D, true, true>(grid, block, s, r);
  } else if (a.goals) {
    rekey<D, true>(grid, block, s, r);
  } else {
    rekey<D, false>(grid, block, s, r);
  }
}

}  // namespace

// The modes are those of launch_open_push (open_kernel.hip) and so are the combinations refused.
hipError_t launch_open_rekey(int dim, const RekeyArgs &r, hipStream_t s) {
  const OpenArgs &a = r.o;
  if (dim != 2 && dim != 3) return hipErrorInvalidValue;
  if (!r.rctl || !r.mirror || a.n_queries < 1) return hipErrorInvalidValue;
  if (a.dyn && (a.dyn != 2 || a.prior_n || (a.goals && !a.dyn_controls))) return hipErrorInvalidValue;  // MPLX_HEUR_ROBUST
  if (a.field_dist && (a.prior_n || !a.field_of_query || a.field_F < 1 || a.field_cells < 1 || !(a.field_res > 0))) return hipErrorInvalidValue;
  if (a.prior_n && (!a.goals || !a.prior_pos || !a.prior_togo || a.prior_cap < 1)) return hipErrorInvalidValue;
  const int64_t n = a.n_bound > 0 ? a.n_bound : 1;  // (an empty table still gets its bound)
  const dim3 per_node((unsigned)((n + kBlock - 1) / kBlock)), per_query((unsigned)((a.n_queries + kBlock - 1) / kBlock)), block(kBlock);
  hipLaunchKernelGGL(open_rekey_reset_kernel, per_query, block, 0, s, r);
  if (dim == 2) rekey_dim<2>(per_node, block, s, r);
  else rekey_dim<3>(per_node, block, s, r);
  hipLaunchKernelGGL(open_rekey_finish_kernel, per_query, block, 0, s, r);
  return hipGetLastError();
}

}  // namespace mplx
