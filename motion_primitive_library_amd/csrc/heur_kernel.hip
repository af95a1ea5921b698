// heur_kernel.hip -- the dynamics-aware heuristic of a batch of resident states (include/mplx_heur.h): one lane per
// state column, heur::robust of csrc/mplx_heur_math.h (or the default's expression), the goal's own lattice state kept
// at 0 (env_base.h:47: the state hashed under the states' flag against the goal hashed under its own).
//
// The device takes DEFAULT and ROBUST only.  REFERENCE goes through cbrt / acos / cos, whose last bits are OCML's here
// and the C library's on the host, and `t < t_bar` turns such a bit into another candidate set; a device key must be a
// pure function of the inputs.
//
// A lane is issue-bound: a few thousand dependent f64 operations (the bisections of a level advance together, so a
// level's intervals overlap in the pipeline), one load per state row and one store.  Every lane of a wave does the same
// work whatever its number of roots: nothing in the root finder branches on data.
#include "mplx_internal.h"
#include "mplx_pair_device.h"
#include "mplx_heur_math.h"

namespace mplx {
namespace {

constexpr int kBlock = 256;

// waypoint.h:93-125 with the control flag at run time, as host::lattice_hash states it
template <int D>
__device__ __forceinline__ uint64_t state_hash(int control, const double *s) {
  uint64_t h = 0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    if (control & 1) dev::fold(h, pair::quantise(s[i], 0.01));
    if (control & 2) dev::fold(h, pair::quantise(s[D + i], 0.1));
    if (control & 4) dev::fold(h, pair::quantise(s[2 * D + i], 0.1));
    if (control & 8) dev::fold(h, pair::quantise(s[3 * D + i], 0.1));
  }
  if (control & 16) dev::fold(h, pair::quantise(s[4 * D], 0.1));
  return h;
}

template <int D>
__global__ __launch_bounds__(kBlock) void heur_eval_kernel(const HeurArgs A) {
  const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= A.n) return;  // n <= stride: the host's bound
  double s[4 * D + 1], g[4 * D + 1];
  double fin = 0;  // 0 while every row read is finite
#pragma unroll
  for (int i = 0; i < 4 * D + 1; i++) {
    s[i] = A.states[(int64_t)i * A.stride + k];
    g[i] = A.goal[i];
    fin = fin + (s[i] - s[i]);
  }
  double h;
  if (A.mode == 2) {  // MPLX_HEUR_ROBUST
    h = heur::robust<D>(s, g, A.control, A.goal_control, A.w, A.v_max);
  } else {
    const double L = heur::linf<D>(s, g);
    h = A.v_max > 0 ? A.w * L / A.v_max : A.w * L;
  }
  if (h == h && fin == 0 && state_hash<D>(A.control, s) == A.goal_hash) h = 0.0;
  A.out[k] = h;
}

}  // namespace

hipError_t launch_heur_eval(int dim, const HeurArgs &a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  if (dim != 2 && dim != 3) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.n + kBlock - 1) / kBlock)), block(kBlock);
  if (dim == 2) hipLaunchKernelGGL(heur_eval_kernel<2>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(heur_eval_kernel<3>, grid, block, 0, s, a);
  return hipGetLastError();
}

}  // namespace mplx
