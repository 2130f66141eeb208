// bs_roofheight.h -- H(p, X, Y) of include/bs_api.h ("roofs", step 5): the one height function of the roof stage
// (height_kernel, bs_roofs_write_obj) and of the solids (bs_solid.hip).  Every translation unit that includes it is
// compiled with -ffp-contract=off for the host and the device, so the f64 sequence below is the same everywhere.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bs {

__host__ __device__ inline int64_t roof_height(const double* n, const int32_t* c, int32_t z_min, int32_t z_max, int64_t X,
                                               int64_t Y)
{
  const double a = n[0] * ((double)X - (double)c[0]), b = n[1] * ((double)Y - (double)c[1]);
  const double t = a + b;
  double z = (double)c[2] - t / n[2];
  if (!(z >= (double)z_min))
    z = (double)z_min;
  if (z > (double)z_max)
    z = (double)z_max;
  return (int64_t)z;
}

}  // namespace bs
