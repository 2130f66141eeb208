// bs_groundrule.h -- "below ground" of a point for the raster, the point assignment and the roofs (include/bs_api.h,
// "ground model"): against the table of bs_set_ground_model while it is set, against the call's ground_th otherwise.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace bs {

struct GroundRule {
  const int32_t* table;  // [height][width] on the device, INT32_MAX = nothing; nullptr while the switch is off
  int32_t width, height, cell, min_height;
  // z < ground_th of the definitions; x, y, z are the point's own coordinates (any value: every index is checked)
  __device__ bool below(int32_t x, int32_t y, int32_t z, double ground_th) const
  {
    if (table && x >= 0 && y >= 0) {
      const int32_t gx = x / cell, gy = y / cell;
      if (gx < width && gy < height) {
        const int32_t g = table[(int64_t)gy * width + gx];
        if (g != INT32_MAX)
          return (int64_t)z < (int64_t)g + min_height;
      }
    }
    return (double)z < ground_th;
  }
};

}  // namespace bs
