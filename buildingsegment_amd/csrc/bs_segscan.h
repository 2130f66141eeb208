// bs_segscan.h -- reductions over the runs of equal key inside one wave of 64 lanes: the run heads come from one ballot,
// the values from segmented scans with __shfl_up.  Used where a per-key figure is reduced before ONE set of global
// atomics per run (bs_facet.hip, bs_outline.hip, bs_simplify.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace bs {

// lane of the head of my run: the highest set bit of `heads` at or below my lane (bit 0 is always set)
__device__ inline int head_lane(unsigned long long heads, int lane) { return 63 - __clzll((long long)(heads & (~0ull >> (63 - lane)))); }
// last lane of my run: one below the next head above me
__device__ inline int tail_lane(unsigned long long heads, int lane)
{
  const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
  return above ? __ffsll((long long)above) - 2 : 63;
}

}  // namespace bs

// segmented inclusive scans over the runs of a wave: lane l takes lane l - o while that lane is still in its run
#define BS_SEG_SCAN(v, op)                           \
  for (int o = 1; o < 64; o <<= 1) {                 \
    const auto t_ = __shfl_up(v, o);                 \
    if (lane - o >= hl)                              \
      v = op(v, t_);                                 \
  }
#define BS_OP_ADD(a, b) ((a) + (b))
#define BS_OP_MIN(a, b) ((a) < (b) ? (a) : (b))
#define BS_OP_MAX(a, b) ((a) > (b) ? (a) : (b))
