// mplx_body_args.h -- what body_api.cpp hands body_kernel.hip (include/mplx_body.h): the ellipsoid, the binned cloud,
// the lists or the set to check.  A header of its own so that the translation units of the other kernels do not see it.
#ifndef MPLX_BODY_ARGS_H
#define MPLX_BODY_ARGS_H

#include "mplx_internal.h"

namespace mplx {

constexpr int32_t kBodyMaxCells = 1 << 22;

// The grid of the last build, written by the device (the host never waits for it; mplx_body_shape reads it back).
struct BodyGrid {
  double origin[3];  // the smallest included coordinate per axis
  double edge;       // cell edge
  int32_t dims[3];   // cells per axis (1 past D)
  int32_t n_cells;
  int32_t n_incl;    // included points
  int32_t pad;
};

// Scratch of a build: order-preserving integer images of the coordinates' minima and maxima, the included count.
struct BodyBox {
  unsigned long long lo[3], hi[3];
  int32_t n_incl;
  int32_t pad;
};

struct BodyCloud {
  const BodyGrid *grid;
  const int32_t *cell_start;  // [n_cells + 1]
  const double *pts;          // [D][n] cell-contiguous (the first n_incl of every row)
  const int32_t *idx;         // [n] original index of a stored point
  int64_t n;
};

struct BodyShape {
  double g, rr, hh, RR, mct2;  // r*r, h*h, (R*R)*1.0000001, min_cos_tilt^2
};

struct BodyBuildArgs {
  const double *xyz;  // [n][D]
  int64_t n;
  double edge0;       // the automatic edge times the forced multiple
  BodyBox *box;
  BodyGrid *grid;
  int32_t *cell_of_point;  // [n]
  int32_t *cell_start;     // [kBodyMaxCells + 1]
  double *pts;
  int32_t *idx;
};
hipError_t launch_body_build(int dim, const BodyBuildArgs &a, hipStream_t s);

struct BodyCheckArgs {
  BodyShape shape;
  BodyCloud cloud;
  const int32_t *count, *action;
  double *cost;
  int64_t n_rows, S;
  const int32_t *parent_id;
  const double *parent_state;  // [4D+2][parent_stride]
  int64_t parent_stride;
  const double *U;
  int32_t nU, udim;
  double dt, ds;     // ds = dt / (double)n_samp
  int32_t n_samp;
  int32_t sp_log2;   // 2^sp_log2 lanes of a wave over a row's entries, the 64 >> sp_log2 groups split an entry's points
  long long *hit;    // [n_rows * S] or null
  unsigned long long *n_blocked;  // or null
};
hipError_t launch_body_check(int dim, int control, const BodyCheckArgs &a, hipStream_t s);

struct BodyPolyArgs {
  BodyShape shape;
  BodyCloud cloud;
  TrajArgs traj;
  int64_t K;
  double step;
  long long *hit;    // [K] or null
  uint8_t *status;   // [K] or null
  unsigned long long *n_hit;  // or null
};
hipError_t launch_body_check_poly(int dim, const BodyPolyArgs &a, hipStream_t s);

}  // namespace mplx
#endif
