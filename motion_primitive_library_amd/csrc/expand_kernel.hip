// expand_kernel.hip -- batched successor expansion for gfx950 (MI355X).
//
// One lane evaluates one (frontier node, control input) pair; a wavefront
// therefore covers 64 consecutive controls of (almost always) one node, so the
// node state is a broadcast load, the control table and every output row are
// read / written as contiguous 512-byte segments, and the 64 map look-ups of a
// sample step fall into one small neighbourhood of the voxel grid.
//
// This is the device side of MPL::env_map<Dim>::get_succ
//   reference include/mpl_planner/env/env_map.h:147-172 (get_succ)
//   reference include/mpl_planner/env/env_map.h:90-132  (traverse_primitive)
// The arithmetic and the rules that keep it bit-identical to the CPU path are
// stated in mplx_pair_device.h; the polynomial (dev::Ax), the lattice hash,
// the heading check and wrap_angle are the shared ones.  The kernel body below
// still spells the steps of pair::Pair out (init, heading_valid, limits_valid,
// classify, in that order and expression for expression): built on the struct
// it is 3 % slower on C4, see the note in mplx_pair_device.h.
// Final outputs stream past L2 (never re-read by this kernel); scratch for the
// compaction stays cached.
#include "mplx_internal.h"
#include "mplx_pair_device.h"

#include <math.h>

namespace mplx {
namespace {

using dev::wrap_angle;
using pair::heading_ok;
using pair::lattice_hash;

constexpr int kBlock = 256;

template <typename T>
__device__ __forceinline__ void st_out(T *p, T v, bool stream) {
  if (stream) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// ------------------------------------------------------------------ the kernel
template <int D, int K, bool YAW>
__global__ __launch_bounds__(kBlock) void expand_kernel(const ExpandArgs A) {
  const int64_t n_slots = A.n_nodes * (int64_t)A.nU;
  const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot >= n_slots) return;
  const int64_t it = slot / A.nU;  // position in the launch; the override pass of the yaw pinning walks a node list
  const int ci = (int)(slot - it * A.nU);
  const int64_t node = (YAW && A.yaw.node_list) ? (int64_t)A.yaw.node_list[it] : it;

  // ---- load the node (broadcast within the wave) and the control (coalesced)
  const double *nd = A.nodes + node;
  const int64_t ns = A.node_stride;
  double cpos[D], cvel[D], cacc[D], cjrk[D];
#pragma unroll
  for (int i = 0; i < D; i++) {
    cpos[i] = nd[(0 * D + i) * ns];
    cvel[i] = (K >= 2) ? nd[(1 * D + i) * ns] : 0.0;
    cacc[i] = (K >= 3) ? nd[(2 * D + i) * ns] : 0.0;
    cjrk[i] = (K >= 4) ? nd[(3 * D + i) * ns] : 0.0;
  }
  const double cyaw = YAW ? nd[(4 * D) * ns] : 0.0;
  const double ct = nd[(4 * D + 1) * ns];
  const double *u = A.U + (int64_t)ci * A.udim;

  const double T = A.dt;
  dev::Ax<K> ax[D];
#pragma unroll
  for (int i = 0; i < D; i++) ax[i].init(cpos[i], cvel[i], cacc[i], cjrk[i], u[i]);
  const double uyaw = YAW ? u[D] : 0.0;

  // ---- successor state tn = pr.evaluate(dt)  (env_map.h:157, primitive.h:321-331)
  double npos[D], nvel[D], nacc[D], njrk[D];
#pragma unroll
  for (int i = 0; i < D; i++) {
    npos[i] = ax[i].template pos<true>(T);
    nvel[i] = ax[i].template vel<true>(T);
    nacc[i] = ax[i].template acc<true>(T);
    njrk[i] = ax[i].template jrk<true>(T);
  }
  double nyaw = 0.0;
  if (YAW) nyaw = wrap_angle((0.0 + uyaw * T) + cyaw);

  const uint64_t h_next = lattice_hash<D, K, YAW>(npos, nvel, nacc, njrk, nyaw);
  const uint64_t h_curr = lattice_hash<D, K, YAW>(cpos, cvel, cacc, cjrk, cyaw);

  // ---- dynamic limits (primitive.h:450-475); max_vel is needed again by the
  //      traversal, so it is computed once here
  double mv[D];
  double max_v = 0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    mv[i] = ax[i].max_vel(T);
    if (mv[i] > max_v) max_v = mv[i];
  }
  bool valid = true;
  if (YAW && A.yaw_max > 0) {
    // override pass (YawPin): per listed node {cos, sin} of yaw(0), then of yaw(T) for every control, and cos(yaw_max),
    // all from the host libm
    const double *tab = A.yaw.tab ? A.yaw.tab + it * A.yaw.tab_stride : nullptr;
    const double cos_lim = tab ? A.yaw.cos_lim : cos(A.yaw_max);
    // evaluate(0): vel = 0.0 + c4 terms, yaw = wrap(0.0 + uyaw*0 + yaw)
    const double y0 = wrap_angle((0.0 + uyaw * 0.0) + cyaw);
    bool amb = false;
    const bool ok0 = heading_ok(ax[0].template vel<true>(0.0), ax[1].template vel<true>(0.0), y0, cos_lim,
                                tab ? tab : nullptr, A.yaw.margin, A.yaw.tie_yaw, &amb);
    const bool okT = heading_ok(nvel[0], nvel[1], nyaw, cos_lim, tab ? tab + 2 + 2 * ci : nullptr, A.yaw.margin,
                                A.yaw.tie_yaw, &amb);
    valid = ok0 && okT;
    if (amb && A.yaw.amb) mplx::dev::flag_node(A.yaw.amb, A.yaw.amb_cap, node, A.yaw.any_host);
  }
  if (K >= 2 && A.v_max > 0) {
#pragma unroll
    for (int i = 0; i < D; i++) valid = valid && !(mv[i] > A.v_max);
  }
  if (K >= 3 && A.a_max > 0) {
#pragma unroll
    for (int i = 0; i < D; i++) valid = valid && !(ax[i].max_acc(T) > A.a_max);
  }
  if (K >= 4 && A.j_max > 0) {
#pragma unroll
    for (int i = 0; i < D; i++) valid = valid && !(ax[i].max_jrk(T) > A.j_max);
  }

  uint8_t st;
  double cost = INFINITY;
  int iters = 0;
  if (h_next == h_curr) {
    st = 0;  // MPLX_SLOT_SKIP_SAME
  } else if (!valid) {
    st = 3;  // MPLX_SLOT_SKIP_DYN
  } else {
    // ---- traverse_primitive (env_map.h:90-132), skipped when the position
    //      does not change at all (env_map.h:163)
    bool same_pos = true;
#pragma unroll
    for (int i = 0; i < D; i++) same_pos = same_pos && (cpos[i] == npos[i]);
    double c = 0;
    bool blocked = false;
    if (!same_pos) {
      int n = (int)ceil(max_v * T / A.res);
      n = n < 5 ? 5 : n;
      const double sdt = T / n;
      const double org[3] = {A.org0, A.org1, A.org2};
      const int dims[3] = {A.dim0, A.dim1, A.dim2};
      const bool want_vel = (A.pot != nullptr && A.grad_w != 0) || (YAW && A.wyaw > 0);
      for (double t = 0; t < T; t += sdt) {
        iters++;
        int cell[D];
        bool outside = false;
#pragma unroll
        for (int i = 0; i < D; i++) {
          // map_util.h:103-108
          cell[i] = (int)round((ax[i].template pos<false>(t) - org[i]) / A.res - 0.5);
          outside = outside || cell[i] < 0 || cell[i] >= dims[i];
        }
        if (outside) { blocked = true; break; }
        int64_t idx = cell[0] + (int64_t)dims[0] * cell[1];
        if (D == 3) idx += (int64_t)dims[0] * dims[1] * cell[2];
        if (A.region != nullptr && !((A.region[idx >> 5] >> (idx & 31)) & 1u)) { blocked = true; break; }
        double vs[D];
        if (want_vel) {
#pragma unroll
          for (int i = 0; i < D; i++) vs[i] = ax[i].template vel<false>(t);
        }
        if (A.pot != nullptr) {
          const int pv = A.pot[idx];
          if (pv < 100 && pv > 0) {
            double gterm = 0;
            if (A.grad_w != 0) {
              double q = 0;
#pragma unroll
              for (int i = 0; i < D; i++) q += vs[i] * vs[i];
              gterm = A.grad_w * sqrt(q);
              c += sdt * (A.pot_w * pv + gterm);
            } else {
              // gradient_weight * norm is an exact +0 when the weight is 0
              c += sdt * (A.pot_w * pv + 0.0);
            }
          } else if (pv >= 100) { blocked = true; break; }
        } else if (A.map[idx] == 100) { blocked = true; break; }
        if (YAW && A.wyaw > 0) {
          double ux, uy;
          if (mplx::dev::heading_unit(vs[0], vs[1], ux, uy)) {  // (mplx_device_common.h: the same unit vector in every kernel)
            const double yw = wrap_angle(uyaw * t + cyaw);
            const double v_value = 1 - (ux * cos(yw) + uy * sin(yw));
            c += A.wyaw * v_value * sdt;
          }
        }
      }
    }
    if (blocked) {
      st = 2;  // MPLX_SLOT_BLOCKED
    } else {
      // env_map.h:164-165, env_base.h:343-345: cost += J + w*dt
      double J = 0;
#pragma unroll
      for (int i = 0; i < D; i++) J += ax[i].effort(T);
      cost = c + (J + A.w * A.dt);
      st = 1;  // MPLX_SLOT_FINITE
    }
  }

  // ---- dense, coalesced slot writes
  // final outputs stream past L2 (never re-read by this kernel); scratch for the compaction stays cached
  const bool stream = A.stream_out != 0;
  const int64_t oslot = node * A.nU + ci;  // == slot except in the override pass of the yaw pinning
  if (A.status) st_out(&A.status[oslot], st, stream);
  if (A.cost) st_out(&A.cost[oslot], cost, stream);
  if (A.hash) st_out(&A.hash[oslot], h_next, stream);
  if (A.iters) st_out(&A.iters[oslot], iters, stream);
  if (A.state) {
    double *o = A.state + oslot;
    const int64_t ss = A.state_stride;
#pragma unroll
    for (int i = 0; i < D; i++) {
      st_out(&o[(0 * D + i) * ss], npos[i], stream);
      st_out(&o[(1 * D + i) * ss], nvel[i], stream);
      st_out(&o[(2 * D + i) * ss], nacc[i], stream);
      st_out(&o[(3 * D + i) * ss], njrk[i], stream);
    }
    st_out(&o[(4 * D) * ss], nyaw, stream);
    st_out(&o[(4 * D + 1) * ss], ct + A.dt, stream);  // env_map.h:161
  }
}

template <int D, int K, bool YAW>
hipError_t launch_one(const ExpandArgs &a, hipStream_t stream) {
  const int64_t n_slots = a.n_nodes * (int64_t)a.nU;
  if (n_slots == 0) return hipSuccess;
  const int64_t blocks = (n_slots + kBlock - 1) / kBlock;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((expand_kernel<D, K, YAW>), dim3((unsigned)blocks), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

template <int D>
hipError_t launch_dim(int control, const ExpandArgs &a, hipStream_t s) {
  switch (control) {
    case 0x01: return launch_one<D, 1, false>(a, s);
    case 0x03: return launch_one<D, 2, false>(a, s);
    case 0x07: return launch_one<D, 3, false>(a, s);
    case 0x0f: return launch_one<D, 4, false>(a, s);
    case 0x11: return launch_one<D, 1, true>(a, s);
    case 0x13: return launch_one<D, 2, true>(a, s);
    case 0x17: return launch_one<D, 3, true>(a, s);
    case 0x1f: return launch_one<D, 4, true>(a, s);
    default: return hipErrorInvalidValue;
  }
}

__global__ void math_probe_kernel(int op, const double *a, const double *b, double *out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = a[i];
  double r;
  switch (op) {
    case 0: r = x / b[i]; break;
    case 1: r = sqrt(x); break;
    case 2: r = cos(x); break;
    case 3: r = sin(x); break;
    case 4: r = round(x); break;
    default: r = ceil(x); break;
  }
  out[i] = r;
}

__global__ void pack_region_kernel(const uint8_t *bytes, uint32_t *bits, int64_t n_cells) {
  const int64_t wordi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n_words = (n_cells + 31) >> 5;
  if (wordi >= n_words) return;
  uint32_t w = 0;
  const int64_t base = wordi << 5;
  for (int k = 0; k < 32; k++) {
    const int64_t c = base + k;
    if (c < n_cells && bytes[c]) w |= (1u << k);
  }
  bits[wordi] = w;
}

// One workgroup per node: ordered compaction of the emitted slots (status 1/2).
__global__ __launch_bounds__(256) void compact_lists_kernel(const CompactArgs A) {
  __shared__ int s_wsum[4];
  const int64_t nl = blockIdx.x;
  const int64_t node = A.node_offset + nl;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int emitted = 0;
  for (int base = 0; base < A.nU; base += 256) {
    const int ci = base + tid;
    const int64_t slot = nl * A.nU + ci;
    uint8_t st = 0;
    if (ci < A.nU) st = A.status[slot];
    const bool emit = (st == 1 || st == 2);
    const unsigned long long m = __ballot(emit);
    const int within = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wsum[wv] = __popcll(m);
    __syncthreads();
    int pre = 0, tot = 0;
    for (int i = 0; i < 4; i++) { const int c = s_wsum[i]; if (i < wv) pre += c; tot += c; }
    __syncthreads();
    if (emit) {
      const int64_t idx = node * A.l_nstride + emitted + pre + within;
      if (A.l_action) __builtin_nontemporal_store(ci, &A.l_action[idx]);
      if (A.l_cost) __builtin_nontemporal_store(A.cost[slot], &A.l_cost[idx]);
      if (A.l_hash) __builtin_nontemporal_store(A.hash[slot], &A.l_hash[idx]);
      if (A.l_iters && A.iters) __builtin_nontemporal_store(A.iters[slot], &A.l_iters[idx]);
      if (A.l_state)
        for (int f = 0; f < A.n_fields; f++)
          __builtin_nontemporal_store(A.state[(int64_t)f * A.chunk_slots + slot], &A.l_state[(int64_t)f * A.l_stride + idx]);
    }
    emitted += tot;
  }
  if (tid == 0 && A.l_count) A.l_count[node] = emitted;
}

}  // namespace

hipError_t launch_compact_lists(const CompactArgs &a, hipStream_t stream) {
  if (a.n_nodes_chunk <= 0) return hipSuccess;
  hipLaunchKernelGGL(compact_lists_kernel, dim3((unsigned)a.n_nodes_chunk), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_expand(int dim, int control, const ExpandArgs &args, hipStream_t stream) {
  if (dim == 2) return launch_dim<2>(control, args, stream);
  if (dim == 3) return launch_dim<3>(control, args, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_math_probe(int op, const double *a, const double *b, double *out, int64_t n,
                             hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int64_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, op, a, b, out, n);
  return hipGetLastError();
}

hipError_t launch_pack_region(const uint8_t *bytes, uint32_t *bits, int64_t n_cells, hipStream_t stream) {
  const int64_t n_words = (n_cells + 31) >> 5;
  if (n_words <= 0) return hipSuccess;
  const int64_t blocks = (n_words + 255) / 256;
  hipLaunchKernelGGL(pack_region_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, bytes, bits, n_cells);
  return hipGetLastError();
}

}  // namespace mplx
