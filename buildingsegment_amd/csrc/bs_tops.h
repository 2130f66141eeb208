// bs_tops.h -- step 1 of the solids (include/bs_api.h, "solids"): the four corner heights of every building pixel, a
// clean copy of the map and the range checks.  Shared by bs_solid.hip and the roof generalisation (bs_generalise.hip),
// which evaluates the tops of every intermediate roof image.
#pragma once

#include "bs_common.h"
#include "bs_roofheight.h"

namespace bs {
namespace {

struct Tables {  // per plane, device: entry p - 1 is plane p
  const double* normal;
  const int32_t* center;
  const int32_t* z_min;
  const int32_t* z_max;
};

// base_z of building c (include/bs_api.h, "per-building bases"): the table of bs_set_building_bases while it is set, the
// call's scalar otherwise.  c is a checked building number.
struct Bases {
  const int32_t* table;
  int32_t scalar;
  __device__ int32_t of(int32_t c) const { return table ? table[c] : scalar; }
};

__global__ __launch_bounds__(256) void tops_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ roof, int w,
                                                   int h, int32_t nb, int32_t npl, Tables t,
                                                   const int32_t* __restrict__ flat, int bin, Bases bases,
                                                   int4* __restrict__ top, int32_t* __restrict__ cmap, int* __restrict__ bad)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)w * h)
    return;
  int32_t c = map[i];
  const int32_t r = roof[i];
  if (c >= nb || r > npl || (r > 0 && c < 0)) {
    atomicOr(bad, 1);
    c = -1;
  }
  int4 v = make_int4(INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN);
  if (c >= 0) {
    const int32_t base = bases.of(c);
    if (r > 0) {
      const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
      const int32_t s = r - 1;
      const double* n = t.normal + 3 * s;
      const int32_t* ce = t.center + 3 * s;
      const int32_t lo = t.z_min[s], hi = t.z_max[s];
      const int64_t X0 = (int64_t)x * bin, Y0 = (int64_t)y * bin;
      v.x = max(base, (int32_t)roof_height(n, ce, lo, hi, X0, Y0));
      v.y = max(base, (int32_t)roof_height(n, ce, lo, hi, X0 + bin, Y0));
      v.z = max(base, (int32_t)roof_height(n, ce, lo, hi, X0, Y0 + bin));
      v.w = max(base, (int32_t)roof_height(n, ce, lo, hi, X0 + bin, Y0 + bin));
    } else {
      v.x = v.y = v.z = v.w = max(base, flat[c]);
    }
  } else {
    c = -1;
  }
  top[i] = v;
  cmap[i] = c;
}

}  // namespace
}  // namespace bs
