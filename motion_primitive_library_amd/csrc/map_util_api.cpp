// map_util_api.cpp -- C ABI of include/mplx_map_util.h: MapUtil<Dim>::dilate, freeUnknown, freeAll and the three
// voxel clouds on the map the context holds on the device (map_util_kernel.hip).  The same protocol as
// mplx_edit_map (map_prep_api.cpp): pending launches are resolved and a resident service kernel is stopped before the
// cells change, and the map never crosses the host link again.
#include "mplx_ctx.h"
#include "../../include/mplx_map_util.h"

#include <algorithm>
#include <array>
#include <cstdlib>
#include <vector>

using namespace mplx_detail;

namespace {

// Points per fill launch of a cloud (staging buffer of 96 MiB at dim 3): the copy back goes through it in windows.
constexpr int64_t kCloudChunk = int64_t(1) << 22;

int begin_map_change(mplx_ctx *c) {
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;  // a pending launch read the old cells
  return svc_stop(c);                          // a resident kernel may hold the old cells in its XCD's L2
}

// What mplx_set_map does to the derived state (mplx_api.cpp): the blocked bits -- and with them the free-box table --
// are rebuilt from the new cells by the next launch.  With a potential map installed they come from THAT map
// (env_map.h:113-118 does not consult the occupancy) and stay as they are.
int end_map_change(mplx_ctx *c, int8_t *h_map_out) {
  if (h_map_out) HIP_TRY(c, hipMemcpyAsync(h_map_out, c->map.p, (size_t)c->n_cells, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!c->has_pot) c->blk_ok = false;
  c->blk_epoch++;
  return MPLX_OK;
}

}  // namespace

extern "C" {

int mplx_map_dilate(mplx_ctx *c, const int32_t *offsets, int32_t n, int8_t *h_map_out) {
  if (!c) return MPLX_ERR_ARG;
  if (n < 0 || (n > 0 && !offsets)) return fail(c, MPLX_ERR_ARG, "mplx_map_dilate: bad arguments");
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "mplx_map_dilate: set the map first");
  MPLX_GUARD_BEGIN
  const int D = c->dim;
  // Offsets that can never join two cells of the map (|o_i| >= d_i) are dropped, the rest deduplicated and grouped by
  // (dy, dz); each group's dx values are cut into runs of consecutive values (at most 33 per run: one 64-bit window).
  std::vector<std::array<int32_t, 3>> o;
  o.reserve((size_t)n);
  for (int32_t i = 0; i < n; i++) {
    std::array<int32_t, 3> v = {0, 0, 0};
    bool inside = true;
    for (int k = 0; k < D; k++) {
      v[k] = offsets[(size_t)i * D + k];
      if (std::llabs((long long)v[k]) >= c->mdim[k]) inside = false;
    }
    if (inside) o.push_back(v);
  }
  auto key = [](const std::array<int32_t, 3> &v) { return std::array<int32_t, 3>{v[2], v[1], v[0]}; };
  std::sort(o.begin(), o.end(), [&](const std::array<int32_t, 3> &a, const std::array<int32_t, 3> &b) { return key(a) < key(b); });
  o.erase(std::unique(o.begin(), o.end()), o.end());
  std::vector<int32_t> runs;  // {dy, dz, b, len} per run
  for (size_t i = 0; i < o.size();) {
    size_t j = i + 1;
    while (j < o.size() && o[j][1] == o[i][1] && o[j][2] == o[i][2] && o[j][0] == o[j - 1][0] + 1 && j - i < 33) j++;
    runs.insert(runs.end(), {o[i][1], o[i][2], o[j - 1][0], (int32_t)(j - i)});
    i = j;
  }
  const int n_runs = (int)(runs.size() / 4);
  if (int rc = begin_map_change(c)) return rc;
  if (n_runs > 0) {
    const int64_t words = mplx::dilate_words_per_row(c->mdim[0]) * c->mdim[1] * c->mdim[2];
    if (int rc = ensure(c, c->prep_a, (size_t)words * 4)) return rc;
    if (int rc = ensure(c, c->prep_lut, runs.size() * sizeof(int32_t))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->prep_lut.p, runs.data(), runs.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, mplx::launch_dilate((int8_t *)c->map.p, c->mdim, c->prep_lut.p, n_runs, (uint32_t *)c->prep_a.p, c->stream));
  }
  return end_map_change(c, h_map_out);  // (also keeps `runs` alive until the copy is through)
  MPLX_GUARD_END(c)
}

int mplx_map_free(mplx_ctx *c, int unknown_only, int8_t *h_map_out) {
  if (!c) return MPLX_ERR_ARG;
  if (unknown_only != 0 && unknown_only != 1) return fail(c, MPLX_ERR_ARG, "mplx_map_free: unknown_only must be 0 or 1");
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "mplx_map_free: set the map first");
  if (int rc = begin_map_change(c)) return rc;
  if (unknown_only) HIP_TRY(c, mplx::launch_free_unknown((int8_t *)c->map.p, c->n_cells, c->stream));
  else HIP_TRY(c, hipMemsetAsync(c->map.p, 0, (size_t)c->n_cells, c->stream));
  return end_map_change(c, h_map_out);
}

int mplx_map_cloud(mplx_ctx *c, int kind, double *xyz, int64_t cap, int64_t *n_out) {
  if (!c) return MPLX_ERR_ARG;
  if (!n_out || cap < 0 || (kind != MPLX_CELL_OCCUPIED && kind != MPLX_CELL_FREE && kind != MPLX_CELL_UNKNOWN))
    return fail(c, MPLX_ERR_ARG, "mplx_map_cloud: bad arguments");
  if (!c->has_map) return fail(c, MPLX_ERR_STATE, "mplx_map_cloud: set the map first");
  if (int rc = bind_device(c)) return rc;
  if (int rc = resolve_pending(c)) return rc;
  const int D = c->dim;
  const int64_t n_col = (int64_t)c->mdim[0] * (D == 3 ? c->mdim[1] : 1);
  const size_t count_bytes = align256((size_t)n_col * 4);
  if (int rc = ensure(c, c->prep_b, count_bytes + (size_t)(n_col + 1) * 8)) return rc;
  int32_t *count = (int32_t *)c->prep_b.p;
  int64_t *offs = (int64_t *)((char *)c->prep_b.p + count_bytes);
  HIP_TRY(c, mplx::launch_cloud_count((const int8_t *)c->map.p, D, c->mdim, kind, count, offs, c->stream));
  int64_t total = 0;
  HIP_TRY(c, hipMemcpyAsync(&total, offs + n_col, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *n_out = total;
  const int64_t n_fill = xyz ? std::min(total, cap) : 0;
  if (n_fill > 0) {
    const int64_t chunk = std::min(n_fill, kCloudChunk);
    if (int rc = ensure(c, c->prep_a, (size_t)chunk * D * 8)) return rc;
    for (int64_t lo = 0; lo < n_fill; lo += chunk) {
      const int64_t hi = std::min(n_fill, lo + chunk);
      HIP_TRY(c, mplx::launch_cloud_fill((const int8_t *)c->map.p, D, c->mdim, kind, offs, lo, hi, c->res, c->origin,
                                         (double *)c->prep_a.p, c->stream));
      HIP_TRY(c, hipMemcpyAsync(xyz + lo * D, c->prep_a.p, (size_t)(hi - lo) * D * 8, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return MPLX_OK;
}

}  // extern "C"
