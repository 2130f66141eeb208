// bs_outline.h -- what the facet outlines (bs_outline.hip) and the simplified outlines built on them (bs_simplify.hip)
// share: the names of the scratch buffers of bs_ctx::ol, the cut and the Wyllie round of the ranking, and the layout of the
// per-ring arrays on the device.  (The host helpers of every stage are bs_host.h's.)  Everything is internal to a
// translation unit.
#pragma once

#include <algorithm>

#include "bs_common.h"
#include "bs_host.h"

namespace bs {
namespace {

constexpr int GRID_CAP = 4096;  // workgroups of the grid-stride pass over the image
constexpr int32_t END = -1;
// scratch of bs_ctx::ol
enum { OL_FLAGS, OL_BASE, OL_TMP, OL_MISC, OL_HNUM, OL_SUCC, OL_VERT, OL_MN0, OL_MN1, OL_NX0, OL_NX1, OL_VAL0, OL_VAL1, OL_ZV,
       OL_DEST, OL_SLOT, OL_KEYS, OL_KEYS2, OL_VALS, OL_VALS2, OL_RSLOT, OL_RING, OL_LRO, OL_IN_LABEL, OL_IN_TOP, OL_OUT_XY,
       OL_OUT_Z, OL_COUNT };
static_assert(OL_COUNT <= (int)(sizeof(bs_ctx::ol) / sizeof(DevBuf)), "bs_ctx::ol is too short");

inline int grid_of(int64_t n) { return (int)std::min<int64_t>(nblk(n, 256), GRID_CAP); }

// ---- rank ----------------------------------------------------------------------------------------------------------------
// the cycle becomes a list that starts at its leader: the half-edge in front of the leader is the tail
__global__ __launch_bounds__(256) void outline_cut_kernel(const int32_t* __restrict__ succ, const int32_t* __restrict__ leader,
                                                          const uint8_t* __restrict__ vert, int32_t n, int32_t* __restrict__ nxt,
                                                          int32_t* __restrict__ val)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t s = succ[i];
  nxt[i] = s == leader[i] ? END : s;
  val[i] = vert[i];
}

// one Wyllie round: val = the vertex half-edges in [i, nxt)
__global__ __launch_bounds__(256) void outline_jump_kernel(const int32_t* __restrict__ nxt, const int32_t* __restrict__ val,
                                                           int32_t n, int32_t* __restrict__ nxt2, int32_t* __restrict__ val2,
                                                           int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t j = nxt[i];
  if (j == END) {
    nxt2[i] = END;
    val2[i] = val[i];
  } else if ((uint32_t)j >= (uint32_t)n) {
    atomicOr(err, 8);
    nxt2[i] = END;
    val2[i] = val[i];
  } else {
    nxt2[i] = nxt[j];
    val2[i] = val[i] + val[j];
  }
}

// ---- rings ---------------------------------------------------------------------------------------------------------------
struct RingOut {  // per ring in the listed order, device
  unsigned long long* length;
  unsigned long long* area2;
  int32_t* bbox;
  int32_t* label;
  int32_t* start;
  int32_t* vertices;
  int32_t* offset;   // [n_rings + 1]
  int32_t* of_slot;  // [n_rings]: the ring of a slot
};
constexpr size_t RING_OUT_BYTES = 2 * 8 + 9 * 4;  // (+ 4 for the last offset)

inline RingOut ring_out_at(void* p, size_t n)
{
  RingOut r;
  r.length = (unsigned long long*)p;
  r.area2 = r.length + n;
  r.bbox = (int32_t*)(r.area2 + n);
  r.label = r.bbox + 4 * n;
  r.start = r.label + n;
  r.vertices = r.start + n;
  r.of_slot = r.vertices + n;
  r.offset = r.of_slot + n;
  return r;
}

inline int rounds_of(int64_t n)  // the smallest R with 2^R >= n
{
  int r = 0;
  while ((1ll << r) < n)
    r++;
  return r;
}

}  // namespace
}  // namespace bs
