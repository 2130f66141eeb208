// bs_hull.hip -- the convex hull and the minimum-area enclosing rectangle of every label of a label image (DESIGN.md
// "Oriented boxes"; the definition is written down in include/bs_api.h under "oriented boxes").  It builds on the plain
// outline count (bs_outline.hip), whose half-edges, leaders and ring figures it reads from the context.
//   labels      box and pixels2 of every label from the ring figures (one lane per ring), hence its status
//   candidates  a hull vertex is a convex vertex of an outer ring: half-edge (p, k) whose predecessor is side k - 1 of the
//               same pixel.  One flag pass, one exclusive sum, one pass that stores label and box-relative corner of every
//               candidate and takes the two seeds of its label with one 64-bit atomicMin and atomicMax of (corner, id)
//   rounds      QuickHull, all labels together.  A hull edge is named by the candidate at its start; nextv[] is its end.
//               Every live candidate carries the edge it lies outside of.  A round = split (every live candidate looks up
//               the farthest point f of its edge a -> b, moves to a -> f or f -> b or retires, and bids for the farthest
//               point of its new edge with one 64-bit atomicMax of (distance << 32 | id)) + apply (f links itself in).
//               The host reads the live count once every BS_HULL_ROUND_BATCH rounds.
//   order       the hull vertices get the key (label, chain, +-corner) -- the chain from the lowest to the highest corner
//               runs by ascending corner, the way back by descending -- and one radix sort puts them in walk order from
//               the lowest corner.  A vertex that is collinear with its neighbours is dropped (a tie of the farthest
//               distance lets one through), an exclusive sum gives the places and hull_offset.
//   boxes       one wave per label: a lane per edge loops over the hull of its label, the lanes reduce to the least
//               rectangle by the exact 128-bit comparison, the lowest edge on a tie, and sum the shoelace terms.
// No thread walks a ring or a hull list.  Every index read from memory is checked before it is used as an address; a
// violation sets err and the call returns BS_ERR_INTERNAL.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bs_chain.h"  // (bad_image)
#include "bs_common.h"
#include "bs_host.h"
#include "bs_outline.h"

namespace bs {
namespace {

// scratch of bs_ctx::hl
enum { HL_MISC, HL_LABEL, HL_HLAB, HL_CPOS, HL_CXY, HL_CLAB, HL_EDGE, HL_CHAIN, HL_NEXT, HL_BEST0, HL_BEST1, HL_LIVE, HL_HPOS,
       HL_KEYS, HL_KEYS2, HL_VALS, HL_VALS2, HL_LO, HL_KEEP, HL_SPOS, HL_HULL, HL_FIG, HL_TMP, HL_IN_LABEL, HL_OUT_XY, HL_COUNT };
static_assert(HL_COUNT <= (int)(sizeof(bs_ctx::hl) / sizeof(DevBuf)), "bs_ctx::hl is too short");

constexpr int32_t LIVE = 0, RETIRED = -1, ON_HULL = -2;  // edge[c] >= LIVE: the edge the candidate lies outside of
constexpr int LIVE_SLOTS = BS_HULL_ROUND_CAP + 2 * BS_HULL_ROUND_BATCH;

struct LabelDev {  // per label, device
  unsigned long long* pix2;  // (two's complement sum)
  unsigned long long* smin;  // (box-relative corner << 32) | candidate: the lowest, the highest
  unsigned long long* smax;
  int32_t* box;
};
constexpr size_t LABEL_DEV_BYTES = 3 * 8 + 4 * 4;

LabelDev label_dev_at(void* p, size_t n)
{
  LabelDev L;
  L.pix2 = (unsigned long long*)p;
  L.smin = L.pix2 + n;
  L.smax = L.smin + n;
  L.box = (int32_t*)(L.smax + n);
  return L;
}

struct FigDev {  // per label, device: the results of the box pass
  long long* area2;
  long long* len2;
  long long* a_min;
  long long* a_max;
  long long* c_max;
  long long* area_num;
  int32_t* best;
  int32_t* dir;   // [n][2]
  int32_t* hoff;  // [n + 1]
};
constexpr size_t FIG_DEV_BYTES = 6 * 8 + 4 * 4;  // (+ 4 for the last offset)

FigDev fig_dev_at(void* p, size_t n)
{
  FigDev F;
  F.area2 = (long long*)p;
  F.len2 = F.area2 + n;
  F.a_min = F.len2 + n;
  F.a_max = F.a_min + n;
  F.c_max = F.a_max + n;
  F.area_num = F.c_max + n;
  F.best = (int32_t*)(F.area_num + n);
  F.dir = F.best + n;
  F.hoff = F.dir + 2 * n;
  return F;
}

__host__ __device__ inline int status_of(const int32_t* box)
{
  if (box[0] == INT32_MAX)
    return BS_HULL_EMPTY;
  return (box[2] - box[0] > BS_HULL_MAX_SIDE || box[3] - box[1] > BS_HULL_MAX_SIDE) ? BS_HULL_TOO_LARGE : BS_HULL_OK;
}

// a box-relative corner is x | y << 16 (both <= BS_HULL_MAX_SIDE)
__device__ inline long long orient(uint32_t a, uint32_t b, uint32_t c)
{
  const long long ax = a & 0xffffu, ay = a >> 16;
  return ((long long)(b & 0xffffu) - ax) * ((long long)(c >> 16) - ay) - ((long long)(b >> 16) - ay) * ((long long)(c & 0xffffu) - ax);
}
__device__ inline uint32_t corner_key(uint32_t p) { return ((p >> 16) << 14) | (p & 0xffffu); }  // ascending (y, x), < 2^28

// a * b < c * d, all four non-negative, in 128 bits
__host__ __device__ inline bool less_product(long long a, long long b, long long c, long long d)
{
#ifdef __HIP_DEVICE_COMPILE__
  const unsigned long long h1 = __umul64hi((unsigned long long)a, (unsigned long long)b), l1 = (unsigned long long)a * (unsigned long long)b;
  const unsigned long long h2 = __umul64hi((unsigned long long)c, (unsigned long long)d), l2 = (unsigned long long)c * (unsigned long long)d;
  return h1 < h2 || (h1 == h2 && l1 < l2);
#else
  return (unsigned __int128)a * (unsigned __int128)b < (unsigned __int128)c * (unsigned __int128)d;
#endif
}

__device__ inline void count_lanes(bool mine, int* counter)  // one atomic per wave
{
  const unsigned long long m = __ballot(mine);
  if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1)
    atomicAdd(counter, __popcll(m));
}

// ---- labels --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hull_label_init_kernel(LabelDev L, int32_t nl)
{
  const int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (l >= nl)
    return;
  L.pix2[l] = 0;
  L.smin[l] = ~0ull;
  L.smax[l] = 0;
  L.box[4 * l] = L.box[4 * l + 1] = INT32_MAX;
  L.box[4 * l + 2] = L.box[4 * l + 3] = INT32_MIN;
}

__global__ __launch_bounds__(256) void hull_ring_kernel(RingOut R, int32_t nr, int32_t nl, LabelDev L, int* __restrict__ err)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nr)
    return;
  const int32_t l = R.label[r];
  if ((uint32_t)l >= (uint32_t)nl) {
    atomicOr(err, 1);
    return;
  }
  const long long a = (long long)R.area2[r];
  atomicAdd(L.pix2 + l, (unsigned long long)a);
  if (a > 0) {
    atomicMin(L.box + 4 * (int64_t)l, R.bbox[4 * r]);
    atomicMin(L.box + 4 * (int64_t)l + 1, R.bbox[4 * r + 1]);
    atomicMax(L.box + 4 * (int64_t)l + 2, R.bbox[4 * r + 2]);
    atomicMax(L.box + 4 * (int64_t)l + 3, R.bbox[4 * r + 3]);
  }
}

// ---- candidates ----------------------------------------------------------------------------------------------------------
// hlab[i] = the label of half-edge i where it is a candidate, else -1
__global__ __launch_bounds__(256) void hull_flag_kernel(const int32_t* __restrict__ hnum, const uint8_t* __restrict__ flags,
                                                        const int32_t* __restrict__ leader, const int32_t* __restrict__ slot,
                                                        RingOut R, LabelDev L, int32_t n, int32_t nr, int32_t nl, int64_t npix,
                                                        int32_t* __restrict__ hlab, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  int32_t out = -1;
  const int32_t hn = hnum[i];
  const int64_t p = hn >> 2;
  if (hn < 0 || p >= npix) {
    atomicOr(err, 2);
  } else if ((flags[p] >> ((hn + 3) & 3)) & 1u) {  // the predecessor is the side before on the same pixel: a convex vertex
    const int32_t ld = leader[i];
    const int32_t s = (uint32_t)ld < (uint32_t)n ? slot[ld] : -1;
    const int32_t r = (uint32_t)s < (uint32_t)nr ? R.of_slot[s] : -1;
    if ((uint32_t)r >= (uint32_t)nr) {
      atomicOr(err, 2);
    } else if ((long long)R.area2[r] > 0) {
      const int32_t l = R.label[r];
      if ((uint32_t)l >= (uint32_t)nl)
        atomicOr(err, 2);
      else if (status_of(L.box + 4 * (int64_t)l) == BS_HULL_OK)
        out = l;
    }
  }
  hlab[i] = out;
}

struct IsCandidate {
  __host__ __device__ int32_t operator()(int32_t l) const { return l >= 0; }
};
using CandIt = hipcub::TransformInputIterator<int32_t, IsCandidate, const int32_t*>;

__global__ __launch_bounds__(256) void hull_cand_kernel(const int32_t* __restrict__ hnum, const int32_t* __restrict__ hlab,
                                                        const int32_t* __restrict__ cpos, LabelDev L, int w, int32_t n,
                                                        int32_t nc, uint32_t* __restrict__ cxy, int32_t* __restrict__ clab,
                                                        int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t l = hlab[i];
  if (l < 0)
    return;
  const int32_t c = cpos[i], hn = hnum[i];
  const int64_t p = hn >> 2;
  const int k = hn & 3;
  const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
  const int rx = x + (k == 1 || k == 2) - L.box[4 * (int64_t)l], ry = y + (k >= 2) - L.box[4 * (int64_t)l + 1];
  if ((uint32_t)c >= (uint32_t)nc || (uint32_t)rx > (uint32_t)BS_HULL_MAX_SIDE || (uint32_t)ry > (uint32_t)BS_HULL_MAX_SIDE) {
    atomicOr(err, 4);
    return;
  }
  const uint32_t pt = (uint32_t)rx | ((uint32_t)ry << 16);
  cxy[c] = pt;
  clab[c] = l;
  const unsigned long long key = ((unsigned long long)corner_key(pt) << 32) | (uint32_t)c;
  atomicMin(L.smin + l, key);
  atomicMax(L.smax + l, key);
}

// the two seeds of a label are the ends of its first two edges
__global__ __launch_bounds__(256) void hull_seed_kernel(LabelDev L, int32_t nl, int32_t nc, int32_t* __restrict__ nextv,
                                                        int* __restrict__ err)
{
  const int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (l >= nl || status_of(L.box + 4 * l) != BS_HULL_OK)
    return;
  const int32_t a = (int32_t)(uint32_t)L.smin[l], b = (int32_t)(uint32_t)L.smax[l];
  if (L.smin[l] == ~0ull || (uint32_t)a >= (uint32_t)nc || (uint32_t)b >= (uint32_t)nc || a == b) {
    atomicOr(err, 8);
    return;
  }
  nextv[a] = b;
  nextv[b] = a;
}

// ---- rounds --------------------------------------------------------------------------------------------------------------
// the first assignment: chain 0 lies outside a -> b (from the lowest corner to the highest), chain 1 outside b -> a
__global__ __launch_bounds__(256) void hull_assign_kernel(const uint32_t* __restrict__ cxy, const int32_t* __restrict__ clab,
                                                          LabelDev L, int32_t nc, int32_t nl, int32_t* __restrict__ edge,
                                                          uint8_t* __restrict__ chain, unsigned long long* __restrict__ best,
                                                          int* __restrict__ live, int* __restrict__ n_hull, int* __restrict__ err)
{
  const int64_t c64 = ((int64_t)nc + 63) & ~(int64_t)63;  // whole waves stay together
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= c64)
    return;
  bool is_live = false, is_hull = false;
  if (c < nc) {
    const int32_t l = clab[c];
    int32_t e = RETIRED;
    uint8_t ch = 0;
    if ((uint32_t)l >= (uint32_t)nl) {
      atomicOr(err, 16);
    } else {
      const int32_t a = (int32_t)(uint32_t)L.smin[l], b = (int32_t)(uint32_t)L.smax[l];
      if ((uint32_t)a >= (uint32_t)nc || (uint32_t)b >= (uint32_t)nc) {
        atomicOr(err, 16);
      } else if (c == a || c == b) {
        e = ON_HULL;
        is_hull = true;
      } else {
        const long long o = orient(cxy[a], cxy[b], cxy[c]);
        if (o != 0) {
          ch = o > 0;
          e = o < 0 ? a : b;
          is_live = true;
          atomicMax(best + e, ((unsigned long long)(o < 0 ? -o : o) << 32) | (uint32_t)c);
        }
      }
    }
    edge[c] = e;
    chain[c] = ch;
  }
  count_lanes(is_live, live);
  count_lanes(is_hull, n_hull);
}

// every live candidate but the farthest of its edge a -> b: to a -> f, to f -> b, or inside the triangle
__global__ __launch_bounds__(256) void hull_split_kernel(const uint32_t* __restrict__ cxy, const int32_t* __restrict__ nextv,
                                                         int32_t nc, int32_t* __restrict__ edge,
                                                         const unsigned long long* __restrict__ cur,
                                                         unsigned long long* __restrict__ nxt, int* __restrict__ live,
                                                         int* __restrict__ err)
{
  const int64_t c64 = ((int64_t)nc + 63) & ~(int64_t)63;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= c64)
    return;
  bool is_live = false;
  const int32_t a = c < nc ? edge[c] : RETIRED;
  if (a >= LIVE) {
    const unsigned long long key = (uint32_t)a < (uint32_t)nc ? cur[a] : 0;
    const int32_t f = (int32_t)(uint32_t)key;
    const int32_t b = key ? nextv[a] : -1;
    if (!key || (uint32_t)f >= (uint32_t)nc || (uint32_t)b >= (uint32_t)nc) {
      atomicOr(err, 32);
      edge[c] = RETIRED;
    } else if (f != (int32_t)c) {
      const uint32_t pa = cxy[a], pf = cxy[f], pb = cxy[b], pc = cxy[c];
      const long long d1 = -orient(pa, pf, pc);
      const long long d2 = d1 > 0 ? 0 : -orient(pf, pb, pc);
      if (d1 > 0) {
        is_live = true;
        atomicMax(nxt + a, ((unsigned long long)d1 << 32) | (uint32_t)c);
      } else if (d2 > 0) {
        is_live = true;
        edge[c] = f;
        atomicMax(nxt + f, ((unsigned long long)d2 << 32) | (uint32_t)c);
      } else {
        edge[c] = RETIRED;
      }
    }
  }
  count_lanes(is_live, live);
}

// the farthest point f of a -> b becomes a hull vertex: a -> f -> b
__global__ __launch_bounds__(256) void hull_apply_kernel(int32_t nc, int32_t* __restrict__ edge, int32_t* __restrict__ nextv,
                                                         unsigned long long* __restrict__ cur, int* __restrict__ n_hull)
{
  const int64_t c64 = ((int64_t)nc + 63) & ~(int64_t)63;
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= c64)
    return;
  bool is_hull = false;
  const int32_t a = c < nc ? edge[c] : RETIRED;
  if (a >= LIVE && (uint32_t)a < (uint32_t)nc) {
    const unsigned long long key = cur[a];  // (the winner alone clears it: the others read this key or 0)
    if (key && (int32_t)(uint32_t)key == (int32_t)c) {
      nextv[c] = nextv[a];
      nextv[a] = (int32_t)c;
      edge[c] = ON_HULL;
      cur[a] = 0;
      is_hull = true;
    }
  }
  count_lanes(is_hull, n_hull);
}

// ---- order ---------------------------------------------------------------------------------------------------------------
struct IsHull {
  __host__ __device__ int32_t operator()(int32_t e) const { return e == ON_HULL; }
};
using HullIt = hipcub::TransformInputIterator<int32_t, IsHull, const int32_t*>;

__global__ __launch_bounds__(256) void hull_keys_kernel(const int32_t* __restrict__ edge, const int32_t* __restrict__ hpos,
                                                        const uint32_t* __restrict__ cxy, const int32_t* __restrict__ clab,
                                                        const uint8_t* __restrict__ chain, int32_t nc, int32_t nh,
                                                        unsigned long long* __restrict__ keys, int32_t* __restrict__ vals,
                                                        int* __restrict__ err)
{
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c >= nc || edge[c] != ON_HULL)
    return;
  const int32_t at = hpos[c];
  if ((uint32_t)at >= (uint32_t)nh) {
    atomicOr(err, 64);
    return;
  }
  const uint32_t ck = corner_key(cxy[c]);
  keys[at] = ((unsigned long long)(uint32_t)clab[c] << 32) | (chain[c] ? 0x80000000u | (0x7fffffffu - ck) : ck);
  vals[at] = (int32_t)c;
}

// lo[l] = the first sorted vertex whose label is >= l: a binary search of `steps` halvings (from the host)
__global__ __launch_bounds__(256) void hull_label_lo_kernel(const unsigned long long* __restrict__ skeys, int32_t nh, int32_t nl,
                                                            int steps, int32_t* __restrict__ lo_of)
{
  const int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (l > nl)
    return;
  int32_t lo = 0, hi = nh;
  for (int s = 0; s < steps; s++) {
    if (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if ((int64_t)(skeys[mid] >> 32) < l)
        lo = mid + 1;
      else
        hi = mid;
    }
  }
  lo_of[l] = lo;
}

__global__ __launch_bounds__(256) void hull_strict_kernel(const unsigned long long* __restrict__ skeys,
                                                          const int32_t* __restrict__ svals, const uint32_t* __restrict__ cxy,
                                                          const int32_t* __restrict__ lo_of, int32_t nh, int32_t nl, int32_t nc,
                                                          uint8_t* __restrict__ keep, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nh)
    return;
  uint8_t k = 0;
  const uint32_t l = (uint32_t)(skeys[i] >> 32);
  if (l >= (uint32_t)nl) {
    atomicOr(err, 128);
  } else {
    const int32_t a = lo_of[l], b = lo_of[l + 1];
    if (a < 0 || b > nh || i < a || i >= b || b - a < 3) {
      atomicOr(err, 128);
    } else {
      const int32_t cp = svals[i == a ? b - 1 : i - 1], cv = svals[i], cn = svals[i + 1 == b ? a : i + 1];
      if ((uint32_t)cp >= (uint32_t)nc || (uint32_t)cv >= (uint32_t)nc || (uint32_t)cn >= (uint32_t)nc) {
        atomicOr(err, 128);
      } else {
        const long long o = orient(cxy[cp], cxy[cv], cxy[cn]);
        if (o < 0)
          atomicOr(err, 256);  // (not convex: the rounds went wrong)
        k = o > 0;
      }
    }
  }
  keep[i] = k;
}

struct KeepCount {  // keep[i], 0 for the entry behind the last
  const uint8_t* keep;
  int32_t nh;
  __host__ __device__ int32_t operator()(int32_t i) const { return i < nh ? keep[i] : 0; }
};

__global__ __launch_bounds__(256) void hull_offset_kernel(const int32_t* __restrict__ lo_of, const int32_t* __restrict__ spos,
                                                          int32_t nh, int32_t nl, int32_t* __restrict__ hoff, int* __restrict__ err)
{
  const int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (l > nl)
    return;
  const int32_t a = lo_of[l];
  if ((uint32_t)a > (uint32_t)nh) {
    atomicOr(err, 512);
    hoff[l] = 0;
  } else {
    hoff[l] = spos[a];
  }
}

__global__ __launch_bounds__(256) void hull_place_kernel(const uint8_t* __restrict__ keep, const int32_t* __restrict__ spos,
                                                         const int32_t* __restrict__ svals, const uint32_t* __restrict__ cxy,
                                                         const int32_t* __restrict__ clab, LabelDev L, int32_t nh, int32_t nc,
                                                         int32_t nl, int2* __restrict__ hxy, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= nh || !keep[i])
    return;
  const int32_t d = spos[i], c = svals[i];
  const int32_t l = (uint32_t)c < (uint32_t)nc ? clab[c] : -1;
  if ((uint32_t)d >= (uint32_t)nh || (uint32_t)l >= (uint32_t)nl) {
    atomicOr(err, 512);
    return;
  }
  const uint32_t p = cxy[c];
  hxy[d] = make_int2(L.box[4 * (int64_t)l] + (int)(p & 0xffffu), L.box[4 * (int64_t)l + 1] + (int)(p >> 16));
}

// ---- boxes ---------------------------------------------------------------------------------------------------------------
__device__ inline long long shfl_xor64(long long v, int m)
{
  const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)v, m), hi = __shfl_xor((int)(v >> 32), m);
  return (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
}

// one wave per label
__global__ __launch_bounds__(256) void hull_box_kernel(const int2* __restrict__ hxy, LabelDev L, int32_t nl, int32_t nh, FigDev F,
                                                       int* __restrict__ err)
{
  const int64_t l = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (l >= nl)
    return;
  const int32_t base = F.hoff[l], m = F.hoff[l + 1] - base;
  const bool ok = status_of(L.box + 4 * l) == BS_HULL_OK;
  const bool sane = base >= 0 && m >= 3 && (int64_t)base + m <= nh;
  if (!ok || !sane) {
    if (ok || m != 0)
      atomicOr(err, 1024);  // (a label within the bound has a hull, the others none)
    if (lane == 0) {
      F.area2[l] = F.len2[l] = F.a_min[l] = F.a_max[l] = F.c_max[l] = F.area_num[l] = 0;
      F.best[l] = F.dir[2 * l] = F.dir[2 * l + 1] = 0;
    }
    return;
  }
  const int32_t bx = L.box[4 * l], by = L.box[4 * l + 1];
  long long shoe = 0, b_num = 0, b_len2 = 0, b_amin = 0, b_amax = 0, b_cmax = 0;
  int32_t b_i = INT32_MAX;
  for (int32_t i = lane; i < m; i += 64) {
    const int2 s = hxy[base + i], e = hxy[base + (i + 1 == m ? 0 : i + 1)];
    const long long dx = e.x - s.x, dy = e.y - s.y, len2 = dx * dx + dy * dy;
    long long amin = 0, amax = 0, cmax = 0;
    for (int32_t j = 0; j < m; j++) {
      const int2 p = hxy[base + j];
      const long long px = p.x - s.x, py = p.y - s.y, a = px * dx + py * dy, c = dx * py - dy * px;
      amin = a < amin ? a : amin;
      amax = a > amax ? a : amax;
      cmax = c > cmax ? c : cmax;
    }
    const long long num = (amax - amin) * cmax;
    shoe += (long long)(s.x - bx) * (e.y - by) - (long long)(e.x - bx) * (s.y - by);  // (from the box's corner: small terms)
    if (b_i == INT32_MAX || less_product(num, b_len2, b_num, len2)) {  // (ascending i: a tie keeps the lower)
      b_i = i, b_num = num, b_len2 = len2, b_amin = amin, b_amax = amax, b_cmax = cmax;
    }
  }
  long long w_num = b_num, w_len2 = b_len2;
  int32_t w_i = b_i;
  for (int off = 32; off >= 1; off >>= 1) {
    const long long o_num = shfl_xor64(w_num, off), o_len2 = shfl_xor64(w_len2, off);
    const int32_t o_i = __shfl_xor(w_i, off);
    shoe += shfl_xor64(shoe, off);
    if (o_i == INT32_MAX)
      continue;
    if (w_i == INT32_MAX || less_product(o_num, w_len2, w_num, o_len2) || (!less_product(w_num, o_len2, o_num, w_len2) && o_i < w_i)) {
      w_i = o_i, w_num = o_num, w_len2 = o_len2;
    }
  }
  if (b_i == w_i) {  // the lane that holds the best edge
    F.area2[l] = shoe;
    F.len2[l] = b_len2;
    F.a_min[l] = b_amin;
    F.a_max[l] = b_amax;
    F.c_max[l] = b_cmax;
    F.area_num[l] = b_num;
    F.best[l] = b_i;
    const int2 s = hxy[base + b_i], e = hxy[base + (b_i + 1 == m ? 0 : b_i + 1)];
    F.dir[2 * l] = e.x - s.x;
    F.dir[2 * l + 1] = e.y - s.y;
  }
}

using Guard = FreeUnlessKept<struct bs_label_hulls, bs_label_hulls_free>;

int internal(bs_ctx* ctx, int err)
{
  char msg[96];
  snprintf(msg, sizeof msg, "oriented boxes: an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

bool alloc_labels(struct bs_label_hulls* r, size_t nl)
{
  return alloc(&r->status, nl) && alloc(&r->box, 4 * nl) && alloc(&r->pixels2, nl) && alloc(&r->n_hull, nl) &&
         alloc(&r->hull_offset, nl + 1) && alloc(&r->hull_area2, nl) && alloc(&r->best_edge, nl) && alloc(&r->dir, 2 * nl) &&
         alloc(&r->len2, nl) && alloc(&r->a_min, nl) && alloc(&r->a_max, nl) && alloc(&r->c_max, nl) && alloc(&r->area_num, nl);
}

bool usable(const struct bs_label_hulls* h, int32_t bin)
{
  return h && bin >= 1 && h->n_labels >= 0 && h->n_hull_vertices >= 0 && h->status && h->hull_offset && h->n_hull && h->dir &&
         h->len2 && h->a_min && h->a_max && h->c_max && h->best_edge && (h->n_hull_vertices == 0 || h->hull_xy);
}

// round(num * bin / len2), half away from zero, one division in 128 bits
int64_t scaled(__int128 num, int32_t bin, int64_t len2)
{
  const __int128 n = num * bin, a = n < 0 ? -n : n;
  const __int128 q = (2 * a + len2) / (2 * (__int128)len2);
  return (int64_t)(n < 0 ? -q : q);
}

int box_corners(const struct bs_label_hulls* h, int32_t l, int32_t bin, const int32_t* origin, int64_t out[4][2])
{
  if (l < 0 || l >= h->n_labels || h->status[l] != BS_HULL_OK || h->len2[l] < 1 || h->best_edge[l] < 0 ||
      h->best_edge[l] >= h->n_hull[l] || h->hull_offset[l] < 0 || h->hull_offset[l] + h->n_hull[l] > h->n_hull_vertices)
    return BS_ERR_INVALID;
  const int32_t* s = h->hull_xy + 2 * (h->hull_offset[l] + h->best_edge[l]);
  const __int128 len2 = h->len2[l], dx = h->dir[2 * l], dy = h->dir[2 * l + 1];
  const __int128 a0 = h->a_min[l], a1 = h->a_max[l], c = h->c_max[l];
  const __int128 kx[4] = {s[0] * len2 + a0 * dx, s[0] * len2 + a1 * dx, s[0] * len2 + a1 * dx - c * dy, s[0] * len2 + a0 * dx - c * dy};
  const __int128 ky[4] = {s[1] * len2 + a0 * dy, s[1] * len2 + a1 * dy, s[1] * len2 + a1 * dy + c * dx, s[1] * len2 + a0 * dy + c * dx};
  for (int k = 0; k < 4; k++) {
    out[k][0] = scaled(kx[k], bin, h->len2[l]) + (origin ? origin[0] : 0);
    out[k][1] = scaled(ky[k], bin, h->len2[l]) + (origin ? origin[1] : 0);
  }
  return BS_OK;
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_label_hulls_free(struct bs_label_hulls* s)
{
  if (!s)
    return;
  free(s->status);
  free(s->box);
  free(s->pixels2);
  free(s->n_hull);
  free(s->hull_offset);
  free(s->hull_area2);
  free(s->best_edge);
  free(s->dir);
  free(s->len2);
  free(s->a_min);
  free(s->a_max);
  free(s->c_max);
  free(s->area_num);
  free(s->hull_xy);
  memset(s, 0, sizeof *s);
}

extern "C" int bs_label_hulls_count_dev(bs_ctx* ctx, const int32_t* d_label, int32_t width, int32_t height, int32_t n_labels,
                                        struct bs_label_hulls* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->hl_valid = false;
  if (!out) {
    ctx->ol_valid = false;
    return fail(ctx, BS_ERR_INVALID, "oriented boxes: null pointer");
  }
  struct bs_outlines plain;
  const int rc = bs_facet_outlines_count_dev(ctx, d_label, nullptr, width, height, n_labels, &plain);
  if (rc != BS_OK)
    return rc;
  const double ms_outlines = plain.ms_halfedges + plain.ms_leaders + plain.ms_rank + plain.ms_rings;
  bs_outlines_free(&plain);

  hipStream_t st = ctx->stream;
  const size_t nl = (size_t)n_labels;
  struct bs_label_hulls res;
  memset(&res, 0, sizeof res);
  Guard guard{&res};
  res.width = width;
  res.height = height;
  res.n_labels = n_labels;
  res.ms_outlines = ms_outlines;
  if (!alloc_labels(&res, nl))
    return fail(ctx, BS_ERR_NOMEM, "oriented boxes: host allocation");
  if (ctx->ol_nhalf == 0 || n_labels == 0) {  // no labelled pixel: every label empty
    for (size_t l = 0; l < nl; l++)
      res.status[l] = BS_HULL_EMPTY;
    res.n_empty = n_labels;
    ctx->hl_nv = 0;
    ctx->hl_valid = true;
    *out = res;
    guard.keep = true;
    return BS_OK;
  }

  const int32_t n = (int32_t)ctx->ol_nhalf, nr = ctx->ol_nr, w = width;
  const int64_t npix = (int64_t)width * height;
  DevBuf* O = ctx->ol;
  DevBuf* B = ctx->hl;
  const int32_t* hnum = O[OL_HNUM].as<int32_t>();
  const uint8_t* flags = O[OL_FLAGS].as<uint8_t>();
  const int32_t* slot = O[OL_SLOT].as<int32_t>();
  const int32_t* leader = ctx->ol_leader;
  const RingOut RO = ring_out_at(O[OL_RING].p, (size_t)nr);
  Events<8> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));

  // ---- labels and candidates ----
  BS_HIP(ctx, B[HL_MISC].reserve(256));
  BS_HIP(ctx, B[HL_LABEL].reserve(LABEL_DEV_BYTES * nl));
  BS_HIP(ctx, B[HL_FIG].reserve(FIG_DEV_BYTES * nl + 4));
  BS_HIP(ctx, B[HL_LIVE].reserve(4 * (size_t)LIVE_SLOTS));
  BS_HIP(ctx, B[HL_LO].reserve(4 * (nl + 1)));
  BS_HIP(ctx, B[HL_HLAB].reserve(4 * (size_t)n));
  BS_HIP(ctx, B[HL_CPOS].reserve(4 * (size_t)n));
  int* d_err = B[HL_MISC].as<int>();
  int* d_nhull = d_err + 1;
  int* d_live = B[HL_LIVE].as<int>();
  int32_t* hlab = B[HL_HLAB].as<int32_t>();
  int32_t* cpos = B[HL_CPOS].as<int32_t>();
  const LabelDev L = label_dev_at(B[HL_LABEL].p, nl);
  const FigDev F = fig_dev_at(B[HL_FIG].p, nl);
  auto scan_cand = [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, CandIt(hlab, IsCandidate()), cpos, n, st);
  };
  BS_HIP(ctx, cub_room(B[HL_TMP], scan_cand));
  BS_HIP(ctx, hipMemsetAsync(d_err, 0, 8, st));
  BS_HIP(ctx, hipMemsetAsync(d_live, 0, 4 * (size_t)LIVE_SLOTS, st));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  hull_label_init_kernel<<<nblk(n_labels, 256), 256, 0, st>>>(L, n_labels);
  hull_ring_kernel<<<nblk(nr, 256), 256, 0, st>>>(RO, nr, n_labels, L, d_err);
  hull_flag_kernel<<<nblk(n, 256), 256, 0, st>>>(hnum, flags, leader, slot, RO, L, n, nr, n_labels, npix, hlab, d_err);
  BS_HIP(ctx, cub_run_sized(B[HL_TMP], scan_cand));
  int h_err = 0;
  int32_t last_pos = 0, last_lab = -1;
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_pos, cpos + n - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_lab, hlab + n - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // round trip 1: n_candidates
  BS_HIP(ctx, hipGetLastError());
  if (h_err)
    return internal(ctx, h_err);
  const int64_t nc64 = (int64_t)last_pos + (last_lab >= 0);
  if (nc64 < 0 || nc64 > n)
    return internal(ctx, 0x10000);
  const int32_t nc = (int32_t)nc64;
  res.n_candidates = nc;

  int32_t nh = 0;
  std::vector<int> h_live;
  if (nc > 0) {
    for (int b : {HL_CXY, HL_CLAB, HL_EDGE, HL_NEXT, HL_HPOS})
      BS_HIP(ctx, B[b].reserve(4 * (size_t)nc));
    BS_HIP(ctx, B[HL_CHAIN].reserve((size_t)nc));
    BS_HIP(ctx, B[HL_BEST0].reserve(8 * (size_t)nc));
    BS_HIP(ctx, B[HL_BEST1].reserve(8 * (size_t)nc));
    uint32_t* cxy = B[HL_CXY].as<uint32_t>();
    int32_t* clab = B[HL_CLAB].as<int32_t>();
    int32_t* edge = B[HL_EDGE].as<int32_t>();
    int32_t* nextv = B[HL_NEXT].as<int32_t>();
    int32_t* hpos = B[HL_HPOS].as<int32_t>();
    uint8_t* chain = B[HL_CHAIN].as<uint8_t>();
    unsigned long long* best[2] = {B[HL_BEST0].as<unsigned long long>(), B[HL_BEST1].as<unsigned long long>()};
    const int ncb = nblk(nc, 256);
    BS_HIP(ctx, hipMemsetAsync(best[0], 0, 8 * (size_t)nc, st));
    BS_HIP(ctx, hipMemsetAsync(best[1], 0, 8 * (size_t)nc, st));
    BS_HIP(ctx, hipMemsetAsync(nextv, 0xff, 4 * (size_t)nc, st));
    hull_cand_kernel<<<nblk(n, 256), 256, 0, st>>>(hnum, hlab, cpos, L, w, n, nc, cxy, clab, d_err);
    hull_seed_kernel<<<nblk(n_labels, 256), 256, 0, st>>>(L, n_labels, nc, nextv, d_err);
    BS_HIP(ctx, hipEventRecord(ev.e[1], st));
    // ---- rounds: live[0] after the first assignment, live[r] after round r ----
    hull_assign_kernel<<<ncb, 256, 0, st>>>(cxy, clab, L, nc, n_labels, edge, chain, best[0], d_live, d_nhull, d_err);
    int r = 0, live_now = 1;
    while (live_now) {
      if (r >= BS_HULL_ROUND_CAP)
        return internal(ctx, 0x20000);
      for (int k = 0; k < BS_HULL_ROUND_BATCH; k++) {
        r++;
        hull_split_kernel<<<ncb, 256, 0, st>>>(cxy, nextv, nc, edge, best[(r - 1) & 1], best[r & 1], d_live + r, d_err);
        hull_apply_kernel<<<ncb, 256, 0, st>>>(nc, edge, nextv, best[(r - 1) & 1], d_nhull);
      }
      BS_HIP(ctx, hipMemcpyAsync(&live_now, d_live + r, 4, hipMemcpyDeviceToHost, st));
      BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
      BS_HIP(ctx, hipMemcpyAsync(&nh, d_nhull, 4, hipMemcpyDeviceToHost, st));
      BS_HIP(ctx, hipStreamSynchronize(st));  // one round trip per batch of rounds
      BS_HIP(ctx, hipGetLastError());
      if (h_err)
        return internal(ctx, h_err);
    }
    BS_HIP(ctx, hipEventRecord(ev.e[2], st));
    h_live.resize((size_t)r + 1);
    BS_HIP(ctx, hipMemcpyAsync(h_live.data(), d_live, 4 * ((size_t)r + 1), hipMemcpyDeviceToHost, st));
    if (nh < 4 || nh > nc)
      return internal(ctx, 0x40000);

    // ---- order ----
    for (int b : {HL_KEYS, HL_KEYS2})
      BS_HIP(ctx, B[b].reserve(8 * (size_t)nh));
    for (int b : {HL_VALS, HL_VALS2})
      BS_HIP(ctx, B[b].reserve(4 * (size_t)nh));
    BS_HIP(ctx, B[HL_KEEP].reserve((size_t)nh));
    BS_HIP(ctx, B[HL_SPOS].reserve(4 * ((size_t)nh + 1)));
    BS_HIP(ctx, B[HL_HULL].reserve(8 * (size_t)nh));
    unsigned long long* keys = B[HL_KEYS].as<unsigned long long>();
    unsigned long long* skeys = B[HL_KEYS2].as<unsigned long long>();
    int32_t* vals = B[HL_VALS].as<int32_t>();
    int32_t* svals = B[HL_VALS2].as<int32_t>();
    int32_t* lo_of = B[HL_LO].as<int32_t>();
    uint8_t* keep = B[HL_KEEP].as<uint8_t>();
    int32_t* spos = B[HL_SPOS].as<int32_t>();
    int2* hxy = B[HL_HULL].as<int2>();
    const int end_bit = 32 + bits_of(n_labels);
    const int nhb = nblk(nh, 256);
    hipcub::CountingInputIterator<int32_t> idx(0);
    hipcub::TransformInputIterator<int32_t, KeepCount, hipcub::CountingInputIterator<int32_t>> kept(idx, KeepCount{keep, nh});
    auto scan_hull = [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, HullIt(edge, IsHull()), hpos, nc, st);
    };
    auto sort = [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, skeys, vals, svals, nh, 0, end_bit, st);
    };
    auto scan_kept = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, kept, spos, nh + 1, st); };
    BS_HIP(ctx, cub_room(B[HL_TMP], scan_hull, sort, scan_kept));
    BS_HIP(ctx, hipEventRecord(ev.e[3], st));
    BS_HIP(ctx, cub_run_sized(B[HL_TMP], scan_hull));
    hull_keys_kernel<<<ncb, 256, 0, st>>>(edge, hpos, cxy, clab, chain, nc, nh, keys, vals, d_err);
    BS_HIP(ctx, cub_run_sized(B[HL_TMP], sort));
    hull_label_lo_kernel<<<nblk((int64_t)n_labels + 1, 256), 256, 0, st>>>(skeys, nh, n_labels, bits_of(nh) + 1, lo_of);
    hull_strict_kernel<<<nhb, 256, 0, st>>>(skeys, svals, cxy, lo_of, nh, n_labels, nc, keep, d_err);
    BS_HIP(ctx, cub_run_sized(B[HL_TMP], scan_kept));
    hull_offset_kernel<<<nblk((int64_t)n_labels + 1, 256), 256, 0, st>>>(lo_of, spos, nh, n_labels, F.hoff, d_err);
    hull_place_kernel<<<nhb, 256, 0, st>>>(keep, spos, svals, cxy, clab, L, nh, nc, n_labels, hxy, d_err);
    BS_HIP(ctx, hipEventRecord(ev.e[4], st));
    // ---- boxes ----
    hull_box_kernel<<<nblk(64 * (int64_t)n_labels, 256), 256, 0, st>>>(hxy, L, n_labels, nh, F, d_err);
    BS_HIP(ctx, hipEventRecord(ev.e[5], st));
    ctx->hl_xy = reinterpret_cast<const int32_t*>(hxy);
  } else {  // every labelled pixel belongs to a label beyond the bound
    BS_HIP(ctx, hipMemsetAsync(B[HL_FIG].p, 0, FIG_DEV_BYTES * nl + 4, st));
    for (int k = 1; k <= 5; k++)
      BS_HIP(ctx, hipEventRecord(ev.e[k], st));
    ctx->hl_xy = nullptr;
  }

  // ---- results ----
  std::vector<int32_t> i32(3 * nl + nl + 1);
  int32_t* h_best = i32.data();
  int32_t* h_dir = h_best + nl;
  int32_t* h_hoff = h_dir + 2 * nl;
  std::vector<long long> pix2(nl);
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.box, L.box, 16 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(pix2.data(), L.pix2, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.hull_area2, F.area2, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.len2, F.len2, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.a_min, F.a_min, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.a_max, F.a_max, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.c_max, F.c_max, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.area_num, F.area_num, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_best, F.best, 4 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_dir, F.dir, 8 * nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_hoff, F.hoff, 4 * (nl + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the last round trip: the results
  BS_HIP(ctx, hipGetLastError());
  if (h_err)
    return internal(ctx, h_err);
  if (h_hoff[0] != 0 || h_hoff[nl] < 0 || h_hoff[nl] > nh)
    return internal(ctx, 0x80000);
  for (size_t l = 0; l < nl; l++) {
    const int s = status_of(res.box + 4 * l);
    res.status[l] = s;
    res.pixels2[l] = s == BS_HULL_EMPTY ? 0 : pix2[l];
    if (s == BS_HULL_EMPTY)
      res.box[4 * l] = res.box[4 * l + 1] = res.box[4 * l + 2] = res.box[4 * l + 3] = 0;
    res.hull_offset[l] = h_hoff[l];
    res.n_hull[l] = h_hoff[l + 1] - h_hoff[l];
    res.best_edge[l] = h_best[l];
    res.dir[2 * l] = h_dir[2 * l];
    res.dir[2 * l + 1] = h_dir[2 * l + 1];
    (s == BS_HULL_OK ? res.n_ok : s == BS_HULL_EMPTY ? res.n_empty : res.n_too_large)++;
    if (res.n_hull[l] < (s == BS_HULL_OK ? 4 : 0) || (s != BS_HULL_OK && res.n_hull[l] != 0))
      return internal(ctx, 0x100000);
  }
  res.hull_offset[nl] = h_hoff[nl];
  res.n_hull_vertices = h_hoff[nl];
  for (size_t k = 0; k < h_live.size(); k++) {
    res.rounds += h_live[k] > 0;
    res.max_live = std::max<int64_t>(res.max_live, h_live[k]);
  }
  res.ms_candidates = ev.ms(0, 1);
  res.ms_rounds = ev.ms(1, 2);
  res.ms_order = ev.ms(3, 4);
  res.ms_boxes = ev.ms(4, 5);
  ctx->hl_nv = res.n_hull_vertices;
  ctx->hl_valid = true;
  *out = res;
  guard.keep = true;
  return BS_OK;
}

extern "C" int bs_label_hulls_emit_dev(bs_ctx* ctx, int32_t* d_hull_xy)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!ctx->hl_valid)
    return fail(ctx, BS_ERR_INVALID, "oriented boxes: emit without a successful count on this context");
  if (ctx->hl_nv > 0 && !d_hull_xy)
    return fail(ctx, BS_ERR_INVALID, "oriented boxes: emit needs d_hull_xy");
  ctx->hl_ms_emit = 0;
  if (ctx->hl_nv == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events<2> ev;
  BS_HIP(ctx, hipEventCreate(&ev.e[0]));
  BS_HIP(ctx, hipEventCreate(&ev.e[1]));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemcpyAsync(d_hull_xy, ctx->hl_xy, 8 * (size_t)ctx->hl_nv, hipMemcpyDeviceToDevice, st));
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  ctx->hl_ms_emit = ev.ms(0, 1);
  return BS_OK;
}

extern "C" int bs_label_hulls(bs_ctx* ctx, const int32_t* label, int32_t width, int32_t height, int32_t n_labels,
                              struct bs_label_hulls* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->hl_valid = ctx->ol_valid = false;
  if (!label || !out || bad_image(width, height) || n_labels < 0)
    return fail(ctx, BS_ERR_INVALID, "oriented boxes: null pointer, width or height < 1, width * height >= 2^29, or n_labels < 0");
  DevBuf* B = ctx->hl;
  Staging S(ctx);
  const int32_t* d_label = S.upload(B[HL_IN_LABEL], label, (size_t)width * height);
  if (!S.ok())
    return S.status();
  struct bs_label_hulls res;
  int rc = bs_label_hulls_count_dev(ctx, d_label, width, height, n_labels, &res);
  if (rc != BS_OK)
    return rc;
  Guard guard{&res};
  const size_t nv = (size_t)res.n_hull_vertices;
  if (!alloc(&res.hull_xy, 2 * nv))
    return fail(ctx, BS_ERR_NOMEM, "oriented boxes: host allocation");
  if (nv > 0) {
    int32_t* d_xy = S.room<int32_t>(B[HL_OUT_XY], 2 * nv);
    if (!S.ok())
      return S.status();
    rc = bs_label_hulls_emit_dev(ctx, d_xy);
    if (rc != BS_OK)
      return rc;
    S.download(res.hull_xy, d_xy, 2 * nv);
    rc = S.finish();
    if (rc != BS_OK)
      return rc;
    res.ms_emit = ctx->hl_ms_emit;
  }
  *out = res;
  guard.keep = true;
  return BS_OK;
}

extern "C" int bs_hull_box_corners(const struct bs_label_hulls* h, int32_t label, int32_t bin, const int32_t* origin,
                                   int64_t out[4][2])
{
  if (!usable(h, bin) || !out)
    return BS_ERR_INVALID;
  return box_corners(h, label, bin, origin, out);
}

// The format is written down in include/bs_api.h.
extern "C" int bs_hull_boxes_write_obj(const struct bs_label_hulls* h, int32_t bin, const int32_t* origin, const char* path)
{
  if (!usable(h, bin) || !path)
    return BS_ERR_INVALID;
  std::vector<int64_t> corners;  // (every label is checked before the file is opened)
  for (int32_t l = 0; l < h->n_labels; l++) {
    if (h->status[l] != BS_HULL_OK)
      continue;
    int64_t k[4][2];
    if (h->n_hull[l] < 3 || box_corners(h, l, bin, origin, k) != BS_OK)
      return BS_ERR_INVALID;
    corners.insert(corners.end(), &k[0][0], &k[0][0] + 8);
  }
  FILE* fo = fopen(path, "w");
  if (!fo)
    return BS_ERR_INVALID;
  const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  fprintf(fo, "# oriented boxes: %d labels, %lld ok, %lld empty, %lld too large, %lld hull vertices\n", h->n_labels,
          (long long)h->n_ok, (long long)h->n_empty, (long long)h->n_too_large, (long long)h->n_hull_vertices);
  long long at = 1;  // the number of the next vertex in the file
  auto polyline = [&](long long n) {
    fputs("l", fo);
    for (long long v = 0; v < n; v++)
      fprintf(fo, " %lld", at + v);
    fprintf(fo, " %lld\n", at);
    at += n;
  };
  size_t kc = 0;
  for (int32_t l = 0; l < h->n_labels; l++) {
    if (h->status[l] != BS_HULL_OK)
      continue;
    fprintf(fo, "g label_%d_hull\n", l);
    for (int64_t v = h->hull_offset[l]; v < h->hull_offset[l] + h->n_hull[l]; v++)
      fprintf(fo, "v %lld %lld %lld\n", (long long)((int64_t)h->hull_xy[2 * v] * bin + org[0]),
              (long long)((int64_t)h->hull_xy[2 * v + 1] * bin + org[1]), (long long)org[2]);
    polyline(h->n_hull[l]);
    fprintf(fo, "g label_%d_box\n", l);
    for (int k = 0; k < 4; k++, kc += 2)
      fprintf(fo, "v %lld %lld %lld\n", (long long)corners[kc], (long long)corners[kc + 1], (long long)org[2]);
    polyline(4);
  }
  const bool ok = !ferror(fo);
  return (fclose(fo) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}
