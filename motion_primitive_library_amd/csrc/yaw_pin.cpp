// yaw_pin.cpp -- heading-limit decisions pinned to the host libm (YawPin, mplx_internal.h): the detection block every
// launch with yaw controls carries (yaw_slot) and the host-side check of what the launches flagged (resolve_pending,
// which re-expands the flagged nodes with the host's trig values).
#include "mplx_ctx.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace mplx_detail;

namespace {

constexpr int kAmbCap = 1023;          // flagged nodes recorded per launch; beyond that the whole launch is re-checked
constexpr int kYawRing = 32;           // launches that may wait for their check
constexpr double kYawMargin = 0x1p-46; // |d - cos(yaw_max)| below this is "within rounding noise": both libraries are
                                       // within a few ulp (2^-53) of the true cos / sin, d is two products and a sum

bool yaw_pin_active(const mplx_ctx *c) {
  return c->tune.yaw_pin && (c->prm.control & 0x10) && c->prm.yaw_max > 0;
}

// cos and sin of one heading the way the reference's binary gets them: primitive.h:519-520 calls cos(w.yaw) and
// sin(w.yaw) in one expression, and GCC (the reference's compiler, at -O1 and above) fuses such a pair into ONE glibc
// sincos() call.  glibc's sincos is not bit-identical to its separate sin() / cos() on every argument (measured: 2 of
// 40 000 threshold headings, profiles/README.md round 2), so the pinning asks sincos() too.  cos(yaw_max) stands
// alone in the reference (primitive.h:521) and stays a plain cos().
void host_sincos(double x, double *s, double *c) { ::sincos(x, s, c); }

double host_wrap(double a) {  // mpl_basis/math.h:15-19
  while (a > M_PI) a -= 2.0 * M_PI;
  while (a < -M_PI) a += 2.0 * M_PI;
  return a;
}

}  // namespace

// The detection block of the next launch: a slot of the ring (older launches are resolved first when it is full).
int mplx_detail::yaw_slot(mplx_ctx *c, mplx::YawPin *y) {
  *y = mplx::YawPin{};
  if (!yaw_pin_active(c)) return MPLX_OK;
  if ((int)c->yaw_pending.size() >= kYawRing)
    if (int rc = mplx_detail::resolve_pending(c)) return rc;
  if (!c->yaw_ring.p) {
    const size_t bytes = (size_t)kYawRing * (1 + kAmbCap) * 4;
    if (int rc = ensure(c, c->yaw_ring, bytes)) return rc;
    HIP_TRY(c, hipMemsetAsync(c->yaw_ring.p, 0, bytes, c->stream));
  }
  if (!c->yaw_any_host) {
    HIP_TRY(c, hipHostMalloc((void **)&c->yaw_any_host, 64, hipHostMallocCoherent));
    *c->yaw_any_host = 0;
  }
  y->any_host = c->yaw_any_host;
  y->amb = (int32_t *)c->yaw_ring.p + c->yaw_pending.size() * (size_t)(1 + kAmbCap);
  y->amb_cap = kAmbCap;
  y->margin = c->tune.yaw_margin > 0 ? c->tune.yaw_margin : kYawMargin;
  {  // is the x-aligned tie exact under THIS host's libm (near_limit, mplx_device_common.h)?
    double sp, cp, sm, cm;
    host_sincos(c->prm.yaw_max, &sp, &cp);
    host_sincos(-c->prm.yaw_max, &sm, &cm);
    const double lim = std::cos(c->prm.yaw_max);
    y->tie_yaw = (cp == lim && cm == lim) ? c->prm.yaw_max : std::nan("");
  }
  return MPLX_OK;
}

namespace {

// Re-expands the nodes `ids` of a pending launch with every trig value of a heading-limit decision taken from the
// HOST libm -- the library the reference itself calls (primitive.h:504-525 -> std::cos / std::sin).
int yaw_fix_pass(mplx_ctx *c, const mplx_ctx::YawPending &p, const int32_t *ids, int64_t n) {
  const int D = c->dim;
  const double *nodes = p.kind == 0 ? p.g.nodes : p.e.nodes;
  const int64_t nstride = p.kind == 0 ? p.g.node_stride : p.e.node_stride;
  const double T = c->prm.dt;
  // the nodes' yaw (row 4D of the frontier; device memory or a pinned host block the kernel read in place)
  std::vector<double> yaw((size_t)n);
  if (n <= 256) {
    for (int64_t k = 0; k < n; k++)
      HIP_TRY(c, hipMemcpyAsync(&yaw[(size_t)k], nodes + (int64_t)(4 * D) * nstride + ids[k], 8, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    int32_t hi = 0;
    for (int64_t k = 0; k < n; k++) hi = ids[k] > hi ? ids[k] : hi;
    std::vector<double> row((size_t)hi + 1);
    HIP_TRY(c, hipMemcpyAsync(row.data(), nodes + (int64_t)(4 * D) * nstride, ((size_t)hi + 1) * 8, hipMemcpyDefault, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t k = 0; k < n; k++) yaw[(size_t)k] = row[(size_t)ids[k]];
  }
  const int nrate = p.kind == 0 ? 16 : c->nU;
  const int stride = 2 + 2 * nrate;
  std::vector<double> tab((size_t)n * stride, 0.0);
  for (int64_t k = 0; k < n; k++) {
    double *t = &tab[(size_t)k * stride];
    const double cyaw = yaw[(size_t)k];
    const double y0 = host_wrap((0.0 + 0.0) + cyaw);  // the yaw polynomial at t = 0 (primitive.h:329, 128-145)
    host_sincos(y0, &t[1], &t[0]);
    if (p.kind == 0) {
      // factorised kernel: [c0, s0, cT[16], sT[16]] over the distinct yaw rates
      for (int j = 0; j < c->u_nd[3] && j < 16; j++) {
        const double yT = host_wrap((0.0 + c->h_uyaw[j] * T) + cyaw);
        host_sincos(yT, &t[2 + 16 + j], &t[2 + j]);
      }
    } else {
      // dense kernel: [c0, s0, {cT, sT} per control]
      for (int i = 0; i < c->nU; i++) {
        const double yT = host_wrap((0.0 + c->h_U[(size_t)i * c->udim + D] * T) + cyaw);
        host_sincos(yT, &t[2 + 2 * i + 1], &t[2 + 2 * i]);
      }
    }
  }
  if (int rc = ensure(c, c->yaw_ids, (size_t)n * 4)) return rc;
  if (int rc = ensure(c, c->yaw_tab, tab.size() * 8)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->yaw_ids.p, ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->yaw_tab.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
  mplx::YawPin y{};
  y.node_list = (const int32_t *)c->yaw_ids.p;
  y.tab = (const double *)c->yaw_tab.p;
  y.tab_stride = stride;
  y.cos_lim = std::cos(c->prm.yaw_max);
  if (p.kind == 0) {
    mplx::GridArgs a = p.g;
    a.n_nodes = n;
    a.yaw = y;
    if (int rc = launch_grid(c, &a)) return rc;
  } else {
    mplx::ExpandArgs a = p.e;
    a.n_nodes = n;
    a.yaw = y;
    HIP_TRY(c, mplx::launch_expand(c->dim, c->prm.control, a, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // `tab` and `ids` leave scope; yaw_ids / yaw_tab are reused
  c->yaw_fix_passes++;
  return MPLX_OK;
}

// A failure after the pending list was swapped out: the ring still holds the counts and ids of launches that are no
// longer pending, and the next launches would start on those slots -- ids beyond their own n_nodes.  Leave no trace.
int resolve_failed(mplx_ctx *c, int rc) {
  c->yaw_pending.clear();
  if (c->yaw_any_host) *c->yaw_any_host = 0;
  if (c->yaw_ring.p) {
    (void)hipStreamSynchronize(c->stream);
    if (hipMemsetAsync(c->yaw_ring.p, 0, c->yaw_ring.cap, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
      release(c->yaw_ring);  // re-allocated (and zeroed) by the next yaw_slot
  }
  return rc;
}

}  // namespace

int mplx_detail::resolve_pending(mplx_ctx *c, bool stream_is_idle) {
  if (c->yaw_pending.empty()) return MPLX_OK;
  MPLX_GUARD_BEGIN
  // several contexts of one process may sit on different GPUs: the fix pass allocates (yaw_ids, yaw_tab) and launches,
  // so the context's device must be the current one whatever entry point came through here
  if (stream_is_idle) {
    // (the caller has just seen the last launch of the stream finish: the common case below needs no runtime call)
    if (c->yaw_any_host && *(volatile int32_t *)c->yaw_any_host == 0) {
      c->yaw_pending.clear();
      return MPLX_OK;
    }
  }
  if (int rc = bind_device(c)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->yaw_any_host && *(volatile int32_t *)c->yaw_any_host == 0) {
    // nothing was flagged by any launch since the last resolve (the common case: the kernels set this pinned word
    // themselves): the lists are final as they are, no copy, no second synchronisation
    c->yaw_pending.clear();
    return MPLX_OK;
  }
  if (c->yaw_any_host) *c->yaw_any_host = 0;
  const size_t np = c->yaw_pending.size(), slot = (size_t)(1 + kAmbCap);
  std::vector<int32_t> ring(np * slot);
  HIP_TRY(c, hipMemcpyAsync(ring.data(), c->yaw_ring.p, ring.size() * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<mplx_ctx::YawPending> pend;
  pend.swap(c->yaw_pending);  // the fix passes launch without detection; nothing new becomes pending meanwhile
  bool any = false;
  for (size_t i = 0; i < np; i++) {
    const int32_t cnt = ring[i * slot];
    if (cnt <= 0) continue;
    any = true;
    const mplx_ctx::YawPending &p = pend[i];
    const int64_t n_all = p.kind == 0 ? p.g.n_nodes : p.e.n_nodes;
    std::vector<int32_t> ids;
    if (cnt <= kAmbCap) {
      ids.assign(ring.begin() + (long)(i * slot + 1), ring.begin() + (long)(i * slot + 1 + cnt));
      std::sort(ids.begin(), ids.end());
      ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    } else {  // more flagged nodes than the block records: re-check the whole launch
      ids.resize((size_t)n_all);
      for (int64_t k = 0; k < n_all; k++) ids[(size_t)k] = (int32_t)k;
    }
    c->yaw_flagged += (int64_t)ids.size();
    const int64_t chunk = 16384;
    for (int64_t k0 = 0; k0 < (int64_t)ids.size(); k0 += chunk) {
      const int64_t nk = std::min<int64_t>(chunk, (int64_t)ids.size() - k0);
      if (int rc = yaw_fix_pass(c, p, ids.data() + k0, nk)) return resolve_failed(c, rc);
    }
  }
  if (any && hipMemsetAsync(c->yaw_ring.p, 0, np * slot * 4, c->stream) != hipSuccess)
    return resolve_failed(c, fail(c, MPLX_ERR_HIP, "resolve_pending: clearing the detection ring failed"));
  return MPLX_OK;
  MPLX_GUARD_END(c)
}
