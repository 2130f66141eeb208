// bs_solid.hip -- a closed, oriented mesh per building from the roof image (DESIGN.md "Solids"; the definition is written
// down in include/bs_api.h under "solids").
//   count   1. tops      one pixel pass: the four corner heights of every building pixel (one 16-byte store), a clean copy
//                        of the map, and the range checks
//           2. vertices  one pass over the lattice corners: the up to 8 (building, height) keys of the four incident
//                        pixels, sorted in registers; the distinct ones are the corner's vertices (count as one byte,
//                        per-building vertex counts in an LDS table)
//           3. faces     one pixel pass: the walls of the pixel and their lengths (faces, indices and crossing walls packed
//                        into 16 bits); a corner is only looked at where a wall has a vertical side
//           4. figures   one streaming pass over top / map / the packed counts (LDS tables flushed once per workgroup,
//                        global atomics from building FIG_CAP on)
//           5. scans     three exclusive sums (hipcub): vertices per corner, faces and indices per pixel
//   emit    vertex pass (one 16-byte store per vertex) and face pass (re-reads the neighbourhood through L1 / L2: every
//           corner of a pixel is sorted again from the four pixels around it)
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_common.h"
#include "bs_host.h"
#include "bs_roofheight.h"
#include "bs_tops.h"

namespace bs {
namespace {

constexpr int FIG_CAP = 1024;  // buildings 0 .. FIG_CAP - 1: figures reduced in LDS (32 KB in figures_kernel)
constexpr int GRID_CAP = 4096; // workgroups of the grid-stride passes
// scratch of bs_ctx::sd
enum { SD_TOP, SD_MAP, SD_CCNT, SD_VOFF, SD_PCNT, SD_FOFF, SD_IOFF, SD_TMP, SD_TAB, SD_FIG, SD_MISC, SD_IN_MAP, SD_IN_ROOF,
       SD_OUT };

inline int grid_of(int64_t n) { return (int)std::min<int64_t>(nblk(n, 256), GRID_CAP); }

constexpr uint64_t NO_KEY = ~0ull;

// (building, height) as one unsigned key: ascending keys = ascending (building, height)
__device__ inline uint64_t key_of(int32_t c, int32_t z) { return ((uint64_t)(uint32_t)c << 32) | ((uint32_t)z ^ 0x80000000u); }
__device__ inline int32_t key_z(uint64_t k) { return (int32_t)((uint32_t)k ^ 0x80000000u); }
__device__ inline int32_t key_c(uint64_t k) { return (int32_t)(k >> 32); }

__device__ inline void cswap(uint64_t& a, uint64_t& b)
{
  const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
  a = lo;
  b = hi;
}

// The keys of lattice corner (X, Y), sorted (Batcher's 19 exchanges; NO_KEY last): every incident building pixel gives
// (c, base_z) and (c, its top at this corner).  map is the clean copy (-1 or a building).
struct Corner {
  uint64_t k0, k1, k2, k3, k4, k5, k6, k7;
  unsigned d;  // bit i: key i is a vertex (valid and not equal to key i - 1)
};

__device__ inline Corner corner_of(const int32_t* __restrict__ map, const int32_t* __restrict__ top, int w, int h, int X, int Y,
                                   Bases base)
{
  Corner K;
  uint64_t* const k[8] = {&K.k0, &K.k1, &K.k2, &K.k3, &K.k4, &K.k5, &K.k6, &K.k7};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int px = X - 1 + (q & 1), py = Y - 1 + (q >> 1);  // this corner is corner (1 - (q & 1), 1 - (q >> 1)) of it
    uint64_t a = NO_KEY, b = NO_KEY;
    if (px >= 0 && px < w && py >= 0 && py < h) {
      const int64_t p = (int64_t)py * w + px;
      const int32_t c = map[p];
      if (c >= 0) {
        a = key_of(c, base.of(c));
        b = key_of(c, top[4 * p + (3 - q)]);
      }
    }
    *k[2 * q] = a;
    *k[2 * q + 1] = b;
  }
  cswap(K.k0, K.k1); cswap(K.k2, K.k3); cswap(K.k4, K.k5); cswap(K.k6, K.k7);
  cswap(K.k0, K.k2); cswap(K.k1, K.k3); cswap(K.k4, K.k6); cswap(K.k5, K.k7);
  cswap(K.k1, K.k2); cswap(K.k5, K.k6);
  cswap(K.k0, K.k4); cswap(K.k1, K.k5); cswap(K.k2, K.k6); cswap(K.k3, K.k7);
  cswap(K.k2, K.k4); cswap(K.k3, K.k5);
  cswap(K.k1, K.k2); cswap(K.k3, K.k4); cswap(K.k5, K.k6);
  K.d = (unsigned)(K.k0 != NO_KEY) | (unsigned)(K.k1 != NO_KEY && K.k1 != K.k0) << 1 |
        (unsigned)(K.k2 != NO_KEY && K.k2 != K.k1) << 2 | (unsigned)(K.k3 != NO_KEY && K.k3 != K.k2) << 3 |
        (unsigned)(K.k4 != NO_KEY && K.k4 != K.k3) << 4 | (unsigned)(K.k5 != NO_KEY && K.k5 != K.k4) << 5 |
        (unsigned)(K.k6 != NO_KEY && K.k6 != K.k5) << 6 | (unsigned)(K.k7 != NO_KEY && K.k7 != K.k6) << 7;
  return K;
}

// bit i: key i < key
__device__ inline unsigned below_mask(const Corner& K, uint64_t key)
{
  return (unsigned)(K.k0 < key) | (unsigned)(K.k1 < key) << 1 | (unsigned)(K.k2 < key) << 2 | (unsigned)(K.k3 < key) << 3 |
         (unsigned)(K.k4 < key) << 4 | (unsigned)(K.k5 < key) << 5 | (unsigned)(K.k6 < key) << 6 | (unsigned)(K.k7 < key) << 7;
}

// f(key, rank) for every vertex of the corner in ascending order
template <class F>
__device__ inline void for_each_vertex(const Corner& K, F f)
{
  int r = 0;
  if (K.d & 1u) { f(K.k0, r); r++; }
  if (K.d & 2u) { f(K.k1, r); r++; }
  if (K.d & 4u) { f(K.k2, r); r++; }
  if (K.d & 8u) { f(K.k3, r); r++; }
  if (K.d & 16u) { f(K.k4, r); r++; }
  if (K.d & 32u) { f(K.k5, r); r++; }
  if (K.d & 64u) { f(K.k6, r); r++; }
  if (K.d & 128u) { f(K.k7, r); r++; }
}

// number of vertices below `key` = the rank of `key` among the corner's vertices
__device__ inline int rank_of(const Corner& K, uint64_t key) { return __popc(K.d & below_mask(K, key)); }

// the vertices of the corner strictly between two heights of building c, as a mask over the sorted keys
__device__ inline unsigned mids_mask(const Corner& K, int32_t c, int32_t za, int32_t zb)
{
  const uint64_t lo = key_of(c, min(za, zb)), hi = key_of(c, max(za, zb));
  return K.d & below_mask(K, hi) & ~below_mask(K, lo + 1);
}

// ---- 1. tops: tops_kernel of bs_tops.h ------------------------------------------------------------------------------

// ---- figures ---------------------------------------------------------------------------------------------------------
struct Fig {  // per building, device
  unsigned long long* pixels;
  unsigned long long* vertices;
  unsigned long long* faces;
  unsigned long long* walls;
  unsigned long long* crossing;
  unsigned long long* volume6;  // (two's complement sums)
  unsigned long long* totals;   // [0] indices
  int32_t* top_min;
  int32_t* top_max;
};

__global__ __launch_bounds__(256) void fig_init_kernel(Fig f, int32_t nb)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < 4)
    f.totals[c] = 0;
  if (c >= nb)
    return;
  f.pixels[c] = f.vertices[c] = f.faces[c] = f.walls[c] = f.crossing[c] = f.volume6[c] = 0;
  f.top_min[c] = INT32_MAX;
  f.top_max[c] = INT32_MIN;
}

// ---- 2. vertices -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void corner_count_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ top,
                                                           int w, int h, Bases base, int32_t nb,
                                                           uint8_t* __restrict__ ccnt, Fig f)
{
  __shared__ unsigned s_nv[FIG_CAP];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x)
    s_nv[k] = 0;
  __syncthreads();
  const int64_t nc = (int64_t)(w + 1) * (h + 1);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nc; i += (int64_t)gridDim.x * blockDim.x) {
    const int Y = (int)(i / (w + 1)), X = (int)(i - (int64_t)Y * (w + 1));
    const Corner K = corner_of(map, top, w, h, X, Y, base);
    for_each_vertex(K, [&](uint64_t k, int) {
      const int32_t c = key_c(k);
      if (c < FIG_CAP)
        atomicAdd(s_nv + c, 1u);
      else
        atomicAdd(f.vertices + c, 1ull);
    });
    ccnt[i] = (uint8_t)__popc(K.d);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x)
    if (s_nv[k])
      atomicAdd(f.vertices + k, (unsigned long long)s_nv[k]);
}

__global__ __launch_bounds__(256) void vertex_emit_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ top,
                                                          int w, int h, int bin, Bases base,
                                                          const int32_t* __restrict__ voff, int4* __restrict__ vertex)
{
  const int64_t nc = (int64_t)(w + 1) * (h + 1);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nc; i += (int64_t)gridDim.x * blockDim.x) {
    const int Y = (int)(i / (w + 1)), X = (int)(i - (int64_t)Y * (w + 1));
    const Corner K = corner_of(map, top, w, h, X, Y, base);
    const int32_t v0 = voff[i];
    const int32_t xm = (int32_t)((int64_t)X * bin), ym = (int32_t)((int64_t)Y * bin);
    for_each_vertex(K, [&](uint64_t k, int r) { vertex[v0 + r] = make_int4(xm, ym, key_z(k), key_c(k)); });
  }
}

// ---- 3. faces --------------------------------------------------------------------------------------------------------
// The neighbour's tops at the two ends of wall edge d of pixel (x, y) of building c; false: the neighbour emits the wall
// (same building, smaller row-major index).  same: the neighbour is a pixel of c.
__device__ inline bool wall_other(const int32_t* __restrict__ map, const int4* __restrict__ top, int w, int h, int x, int y,
                                  int32_t c, int d, Bases base, int32_t* bs, int32_t* be)
{
  const int nx = x + (d == 1) - (d == 3), ny = y + (d == 2) - (d == 0);
  *bs = *be = base.of(c);
  if (nx < 0 || nx >= w || ny < 0 || ny >= h)
    return true;
  const int64_t q = (int64_t)ny * w + nx;
  if (map[q] != c)
    return true;
  if (d == 0 || d == 3)
    return false;
  const int4 t = top[q];
  if (d == 1) {  // s = (x + 1, y) is its 00, e = (x + 1, y + 1) its 01
    *bs = t.x;
    *be = t.z;
  } else {       // d == 2: s = (x + 1, y + 1) is its 10, e = (x, y + 1) its 00
    *bs = t.y;
    *be = t.x;
  }
  return true;
}

// corner (i, j) of the pixel as s and e of wall d, and the pixel's own tops there
#define BS_WALL_ENDS(d, T, si, sj, ei, ej, as, ae)                         \
  const int si = (d == 1 || d == 2), sj = (d == 2 || d == 3);              \
  const int ei = (d == 0 || d == 1), ej = (d == 1 || d == 2);              \
  const int32_t as = d == 0 ? T.x : d == 1 ? T.y : d == 2 ? T.w : T.z;     \
  const int32_t ae = d == 0 ? T.y : d == 1 ? T.w : d == 2 ? T.z : T.x;

// faces | indices << 3 | crossing walls << 9 of every pixel
__global__ __launch_bounds__(256) void face_count_kernel(const int32_t* __restrict__ map, const int4* __restrict__ top, int w,
                                                         int h, Bases base, uint16_t* __restrict__ pcnt)
{
  const int64_t npix = (int64_t)w * h;
  const int32_t* top1 = reinterpret_cast<const int32_t*>(top);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = map[i];
    unsigned packed = 0;
    if (c >= 0) {
      const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
      const int4 T = top[i];
      int nf = 3, ni = 10, ncross = 0;
#pragma unroll
      for (int d = 0; d < 4; d++) {
        BS_WALL_ENDS(d, T, si, sj, ei, ej, as, ae)
        int32_t bs, be;
        if (!wall_other(map, top, w, h, x, y, c, d, base, &bs, &be) || (as == bs && ae == be))
          continue;
        nf++;
        ni += 2 + (as != bs) + (ae != be);
        if (as != bs)
          ni += __popc(mids_mask(corner_of(map, top1, w, h, x + si, y + sj, base), c, as, bs));
        if (ae != be)
          ni += __popc(mids_mask(corner_of(map, top1, w, h, x + ei, y + ej, base), c, ae, be));
        ncross += (as > bs && ae < be) || (as < bs && ae > be);
      }
      packed = (unsigned)nf | ((unsigned)ni << 3) | ((unsigned)ncross << 9);
    }
    pcnt[i] = (uint16_t)packed;
  }
}

struct FaceOut {
  int32_t* offset;
  int32_t* index;
  int32_t* building;
  uint8_t* kind;
};

// What the face pass keeps of a corner of its pixel (building c, the pixel's top there: tz).  The corner is the s of one
// wall of the pixel (the other side's height there: zs) and the e of another (ze): the vertex numbers of base_z, tz, zs
// and ze, and the vertices strictly between tz and zs / ze as masks over the corner's sorted keys.
struct CornerIds {
  int32_t v0, base, top, os, oe;
  unsigned d, ms, me;
};

__device__ inline CornerIds corner_ids(const int32_t* __restrict__ map, const int32_t* __restrict__ top, int w, int h, int X,
                                       int Y, Bases base, int32_t v0, int32_t c, int32_t tz, int32_t zs, int32_t ze)
{
  const Corner K = corner_of(map, top, w, h, X, Y, base);
  CornerIds r;
  r.v0 = v0;
  r.d = K.d;
  r.base = v0 + rank_of(K, key_of(c, base.of(c)));
  r.top = v0 + rank_of(K, key_of(c, tz));
  r.os = v0 + rank_of(K, key_of(c, zs));
  r.oe = v0 + rank_of(K, key_of(c, ze));
  r.ms = mids_mask(K, c, tz, zs);
  r.me = mids_mask(K, c, tz, ze);
  return r;
}

// the vertices of mask m (at most two) of a corner, upwards or downwards
__device__ inline void emit_mids(int32_t v0, unsigned d, unsigned m, bool up, int32_t* __restrict__ index, int32_t& pos)
{
  while (m) {
    const int i = up ? __ffs((int)m) - 1 : 31 - __clz((int)m);
    index[pos++] = v0 + __popc(d & ((1u << i) - 1u));
    m &= ~(1u << i);
  }
}

// one wall: s and e are the pixel's corners at its ends, as / ae the pixel's tops and bs / be the other side's there
__device__ inline void emit_wall(const CornerIds& s, const CornerIds& e, int32_t as, int32_t ae, int32_t bs, int32_t be,
                                 int32_t c, const FaceOut& o, int32_t& f, int32_t& pos)
{
  if (as == bs && ae == be)
    return;
  o.offset[f] = pos;
  o.building[f] = c;
  o.kind[f] = 2;
  f++;
  o.index[pos++] = e.top;
  o.index[pos++] = s.top;
  if (as != bs) {
    emit_mids(s.v0, s.d, s.ms, as < bs, o.index, pos);
    o.index[pos++] = s.os;
  }
  if (ae != be) {
    o.index[pos++] = e.oe;
    emit_mids(e.v0, e.d, e.me, be < ae, o.index, pos);
  }
}

__global__ __launch_bounds__(256) void face_emit_kernel(const int32_t* __restrict__ map, const int4* __restrict__ top, int w,
                                                        int h, Bases base, const int32_t* __restrict__ voff,
                                                        const int32_t* __restrict__ foff, const int32_t* __restrict__ ioff,
                                                        int32_t n_faces, int32_t n_indices, FaceOut o)
{
  const int64_t npix = (int64_t)w * h;
  const int32_t* top1 = reinterpret_cast<const int32_t*>(top);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    o.offset[n_faces] = n_indices;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t c = map[i];
    if (c < 0)
      continue;
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    const int4 T = top[i];
    // the other side of the four walls (a wall the neighbour emits: the pixel's own tops, so that it does not exist here)
    int32_t bs0, be0, bs1, be1, bs2, be2, bs3, be3;
    if (!wall_other(map, top, w, h, x, y, c, 0, base, &bs0, &be0)) { bs0 = T.x; be0 = T.y; }
    if (!wall_other(map, top, w, h, x, y, c, 1, base, &bs1, &be1)) { bs1 = T.y; be1 = T.w; }
    if (!wall_other(map, top, w, h, x, y, c, 2, base, &bs2, &be2)) { bs2 = T.w; be2 = T.z; }
    if (!wall_other(map, top, w, h, x, y, c, 3, base, &bs3, &be3)) { bs3 = T.z; be3 = T.x; }
    const int64_t c00 = (int64_t)y * (w + 1) + x;
    // corner 00 is the s of wall 0 and the e of wall 3, 10 of walls 1 and 0, 11 of walls 2 and 1, 01 of walls 3 and 2
    const CornerIds k00 = corner_ids(map, top1, w, h, x, y, base, voff[c00], c, T.x, bs0, be3);
    const CornerIds k10 = corner_ids(map, top1, w, h, x + 1, y, base, voff[c00 + 1], c, T.y, bs1, be0);
    const CornerIds k11 = corner_ids(map, top1, w, h, x + 1, y + 1, base, voff[c00 + w + 2], c, T.w, bs2, be1);
    const CornerIds k01 = corner_ids(map, top1, w, h, x, y + 1, base, voff[c00 + w + 1], c, T.z, bs3, be2);
    int32_t f = foff[i], pos = ioff[i];
    o.offset[f] = pos;
    o.offset[f + 1] = pos + 3;
    o.offset[f + 2] = pos + 6;
    o.building[f] = o.building[f + 1] = o.building[f + 2] = c;
    o.kind[f] = o.kind[f + 1] = 0;
    o.kind[f + 2] = 1;
    f += 3;
    int32_t* const ix = o.index;
    ix[pos] = k00.top; ix[pos + 1] = k10.top; ix[pos + 2] = k11.top;
    ix[pos + 3] = k00.top; ix[pos + 4] = k11.top; ix[pos + 5] = k01.top;
    ix[pos + 6] = k00.base; ix[pos + 7] = k01.base; ix[pos + 8] = k11.base; ix[pos + 9] = k10.base;
    pos += 10;
    emit_wall(k00, k10, T.x, T.y, bs0, be0, c, o, f, pos);
    emit_wall(k10, k11, T.y, T.w, bs1, be1, c, o, f, pos);
    emit_wall(k11, k01, T.w, T.z, bs2, be2, c, o, f, pos);
    emit_wall(k01, k00, T.z, T.x, bs3, be3, c, o, f, pos);
  }
}

// ---- 4. figures ------------------------------------------------------------------------------------------------------
__device__ inline void fig_global(const Fig& f, int32_t c, unsigned pix, unsigned faces, unsigned walls, unsigned cross,
                                  int32_t mn, int32_t mx, unsigned long long vol)
{
  atomicAdd(f.pixels + c, (unsigned long long)pix);
  atomicAdd(f.faces + c, (unsigned long long)faces);
  if (walls)
    atomicAdd(f.walls + c, (unsigned long long)walls);
  if (cross)
    atomicAdd(f.crossing + c, (unsigned long long)cross);
  atomicMin(f.top_min + c, mn);
  atomicMax(f.top_max + c, mx);
  atomicAdd(f.volume6 + c, vol);
}

__global__ __launch_bounds__(256) void figures_kernel(const int32_t* __restrict__ map, const int4* __restrict__ top,
                                                      const uint16_t* __restrict__ pcnt, int64_t npix, Bases base,
                                                      int32_t nb, Fig f)
{
  __shared__ unsigned s_pix[FIG_CAP], s_faces[FIG_CAP], s_walls[FIG_CAP], s_cross[FIG_CAP];
  __shared__ int s_mn[FIG_CAP], s_mx[FIG_CAP];
  __shared__ unsigned long long s_vol[FIG_CAP];
  __shared__ unsigned long long s_ind;
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    s_pix[k] = s_faces[k] = s_walls[k] = s_cross[k] = 0;
    s_mn[k] = INT32_MAX;
    s_mx[k] = INT32_MIN;
    s_vol[k] = 0;
  }
  if (threadIdx.x == 0)
    s_ind = 0;
  __syncthreads();
  const int64_t npix64 = (npix + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix64; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t c = -1;
    unsigned faces = 0, walls = 0, cross = 0, ind = 0;
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    unsigned long long vol = 0;
    if (i < npix)
      c = map[i];
    if (c >= 0) {
      const int4 T = top[i];
      const unsigned p = pcnt[i];
      faces = p & 7u;
      walls = faces - 3u;
      ind = (p >> 3) & 63u;
      cross = p >> 9;
      mn = min(min(T.x, T.y), min(T.z, T.w));
      mx = max(max(T.x, T.y), max(T.z, T.w));
      vol = (unsigned long long)(2ll * T.x + 2ll * T.w + (long long)T.y + (long long)T.z - 6ll * base.of(c));
    }
    unsigned isum = ind;
    for (int o = 32; o > 0; o >>= 1)
      isum += __shfl_xor(isum, o);
    if ((threadIdx.x & 63) == 0 && isum)
      atomicAdd(&s_ind, (unsigned long long)isum);
    const int32_t c0 = __shfl(c, 0);
    if (__all(c == c0)) {  // the whole wave inside one building (or outside all): reduce in registers
      if (c0 < 0)
        continue;
      for (int o = 32; o > 0; o >>= 1) {
        faces += __shfl_xor(faces, o);
        walls += __shfl_xor(walls, o);
        cross += __shfl_xor(cross, o);
        mn = min(mn, __shfl_xor(mn, o));
        mx = max(mx, __shfl_xor(mx, o));
        vol += __shfl_xor(vol, o);
      }
      if ((threadIdx.x & 63) == 0) {
        if (c0 < FIG_CAP) {
          atomicAdd(s_pix + c0, 64u);
          atomicAdd(s_faces + c0, faces);
          atomicAdd(s_walls + c0, walls);
          atomicAdd(s_cross + c0, cross);
          atomicMin(s_mn + c0, mn);
          atomicMax(s_mx + c0, mx);
          atomicAdd(s_vol + c0, vol);
        } else {
          fig_global(f, c0, 64u, faces, walls, cross, mn, mx, vol);
        }
      }
    } else if (c >= 0) {
      if (c < FIG_CAP) {
        atomicAdd(s_pix + c, 1u);
        atomicAdd(s_faces + c, faces);
        if (walls)
          atomicAdd(s_walls + c, walls);
        if (cross)
          atomicAdd(s_cross + c, cross);
        atomicMin(s_mn + c, mn);
        atomicMax(s_mx + c, mx);
        atomicAdd(s_vol + c, vol);
      } else {
        fig_global(f, c, 1u, faces, walls, cross, mn, mx, vol);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x)
    if (s_pix[k])
      fig_global(f, k, s_pix[k], s_faces[k], s_walls[k], s_cross[k], s_mn[k], s_mx[k], s_vol[k]);
  if (threadIdx.x == 0 && s_ind)
    atomicAdd(f.totals, s_ind);
}

// ---- 5. scans --------------------------------------------------------------------------------------------------------
struct ByteCount {
  __host__ __device__ int32_t operator()(uint8_t v) const { return v; }
};
struct FaceCount {
  __host__ __device__ int32_t operator()(uint16_t v) const { return v & 7; }
};
struct IndexCount {
  __host__ __device__ int32_t operator()(uint16_t v) const { return (v >> 3) & 63; }
};
using CornerIt = hipcub::TransformInputIterator<int32_t, ByteCount, const uint8_t*>;
using FaceIt = hipcub::TransformInputIterator<int32_t, FaceCount, const uint16_t*>;
using IndexIt = hipcub::TransformInputIterator<int32_t, IndexCount, const uint16_t*>;

bool alloc_solids(struct bs_solids* s, int32_t nb)
{
  const size_t m = (size_t)std::max(nb, 1);
  s->pixels = (int64_t*)calloc(m, 8);
  s->vertices = (int64_t*)calloc(m, 8);
  s->faces = (int64_t*)calloc(m, 8);
  s->wall_faces = (int64_t*)calloc(m, 8);
  s->crossing_walls = (int64_t*)calloc(m, 8);
  s->top_min = (int32_t*)calloc(m, 4);
  s->top_max = (int32_t*)calloc(m, 4);
  s->volume6 = (int64_t*)calloc(m, 8);
  return s->pixels && s->vertices && s->faces && s->wall_faces && s->crossing_walls && s->top_min && s->top_max &&
         s->volume6;
}

// (the corners are counted in 32 bits too)
bool bad_image(int32_t w, int32_t h) { return w < 1 || h < 1 || ((int64_t)w + 1) * ((int64_t)h + 1) >= (1ll << 31); }

const char* const SOLIDS_INVALID =
    "solids: null pointer, width or height < 1, n_buildings or n_planes < 0, or bin < 1";

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_solids_free(struct bs_solids* s)
{
  if (!s)
    return;
  free(s->pixels);
  free(s->vertices);
  free(s->faces);
  free(s->wall_faces);
  free(s->crossing_walls);
  free(s->top_min);
  free(s->top_max);
  free(s->volume6);
  free(s->vertex);
  free(s->face_offset);
  free(s->face_index);
  free(s->face_building);
  free(s->face_kind);
  memset(s, 0, sizeof *s);
}

extern "C" int bs_solids_count_dev(bs_ctx* ctx, const int32_t* d_map, const int32_t* d_roof, int32_t width, int32_t height,
                                   int32_t n_buildings, int32_t n_planes, const double* normal, const int32_t* center,
                                   const int32_t* z_min, const int32_t* z_max, int32_t bin, int32_t base_z,
                                   const int32_t* flat, int32_t* d_top, struct bs_solids* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->sd_valid = false;
  if (out)
    memset(out, 0, sizeof *out);
  if (!d_map || !d_roof || !out || bad_image(width, height) || n_buildings < 0 || n_planes < 0 || bin < 1 ||
      (n_buildings > 0 && !flat) || (n_planes > 0 && (!normal || !center || !z_min || !z_max)))
    return fail(ctx, BS_ERR_INVALID, SOLIDS_INVALID);
  const int32_t* d_bases = nullptr;
  if (const int rc = building_bases(ctx, n_buildings, "solids", &d_bases))
    return rc;
  const Bases bases{d_bases, base_z};
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int w = width, h = height;
  const int32_t nb = n_buildings, npl = n_planes;
  const int64_t npix = (int64_t)w * h, nc = (int64_t)(w + 1) * (h + 1);
  const size_t mp = (size_t)std::max(npl, 1), mb = (size_t)std::max(nb, 1);
  DevBuf* B = ctx->sd;
  Events<7> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));

  BS_HIP(ctx, B[SD_TOP].reserve(16 * (size_t)npix));
  BS_HIP(ctx, B[SD_MAP].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[SD_CCNT].reserve((size_t)nc));
  BS_HIP(ctx, B[SD_VOFF].reserve(4 * (size_t)nc));
  BS_HIP(ctx, B[SD_PCNT].reserve(2 * (size_t)npix));
  BS_HIP(ctx, B[SD_FOFF].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[SD_IOFF].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[SD_TAB].reserve(44 * mp + 4 * mb));
  BS_HIP(ctx, B[SD_FIG].reserve(56 * mb + 64));
  BS_HIP(ctx, B[SD_MISC].reserve(256));
  int4* top = B[SD_TOP].as<int4>();
  const int32_t* top1 = B[SD_TOP].as<int32_t>();
  int32_t* cmap = B[SD_MAP].as<int32_t>();
  uint8_t* ccnt = B[SD_CCNT].as<uint8_t>();
  int32_t* voff = B[SD_VOFF].as<int32_t>();
  uint16_t* pcnt = B[SD_PCNT].as<uint16_t>();
  int32_t* foff = B[SD_FOFF].as<int32_t>();
  int32_t* ioff = B[SD_IOFF].as<int32_t>();
  int* d_bad = B[SD_MISC].as<int>();
  // the scans of the mesh offsets, run once the counts are checked
  auto scan = [st](auto counts, int32_t* sums, int64_t n) {
    return [=](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, counts, sums, (int)n, st); };
  };
  auto scan_v = scan(CornerIt(ccnt, ByteCount()), voff, nc);
  auto scan_f = scan(FaceIt(pcnt, FaceCount()), foff, npix);
  auto scan_i = scan(IndexIt(pcnt, IndexCount()), ioff, npix);
  BS_HIP(ctx, cub_room(B[SD_TMP], scan_v, scan_f, scan_i));
  double* tab_normal = B[SD_TAB].as<double>();
  int32_t* tab_center = reinterpret_cast<int32_t*>(tab_normal + 3 * mp);
  int32_t* tab_zmin = tab_center + 3 * mp;
  int32_t* tab_zmax = tab_zmin + mp;
  int32_t* tab_flat = tab_zmax + mp;
  const Tables tab{tab_normal, tab_center, tab_zmin, tab_zmax};
  Fig f;
  f.pixels = B[SD_FIG].as<unsigned long long>();
  f.vertices = f.pixels + mb;
  f.faces = f.vertices + mb;
  f.walls = f.faces + mb;
  f.crossing = f.walls + mb;
  f.volume6 = f.crossing + mb;
  f.totals = f.volume6 + mb;
  f.top_min = reinterpret_cast<int32_t*>(f.totals + 4);
  f.top_max = f.top_min + mb;
  if (npl > 0) {
    BS_HIP(ctx, hipMemcpyAsync(tab_normal, normal, 24 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_center, center, 12 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_zmin, z_min, 4 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_zmax, z_max, 4 * (size_t)npl, hipMemcpyHostToDevice, st));
  }
  if (nb > 0)
    BS_HIP(ctx, hipMemcpyAsync(tab_flat, flat, 4 * (size_t)nb, hipMemcpyHostToDevice, st));

  // ---- tops (into the context: nothing of the caller's is written before the checks have passed) ----
  BS_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, st));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  tops_kernel<<<nblk(npix, 256), 256, 0, st>>>(d_map, d_roof, w, h, nb, npl, tab, tab_flat, bin, bases, top, cmap, d_bad);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  int h_bad = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_bad)
    return fail(ctx, BS_ERR_RANGE,
                "solids: a map value >= n_buildings, a roof value > n_planes, or a roof > 0 outside every building");

  // ---- vertices, faces, figures ----
  fig_init_kernel<<<nblk(std::max<int32_t>(nb, 4), 256), 256, 0, st>>>(f, nb);
  corner_count_kernel<<<grid_of(nc), 256, 0, st>>>(cmap, top1, w, h, bases, nb, ccnt, f);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  face_count_kernel<<<grid_of(npix), 256, 0, st>>>(cmap, top, w, h, bases, pcnt);
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  figures_kernel<<<grid_of(npix), 256, 0, st>>>(cmap, top, pcnt, npix, bases, nb, f);
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));

  if (!alloc_solids(out, nb)) {
    bs_solids_free(out);
    return fail(ctx, BS_ERR_NOMEM, "solids: host allocation");
  }
  unsigned long long tot[4] = {0, 0, 0, 0};
  BS_HIP(ctx, hipMemcpyAsync(tot, f.totals, 32, hipMemcpyDeviceToHost, st));
  if (nb > 0) {
    BS_HIP(ctx, hipMemcpyAsync(out->pixels, f.pixels, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->vertices, f.vertices, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->faces, f.faces, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->wall_faces, f.walls, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->crossing_walls, f.crossing, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->volume6, f.volume6, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->top_min, f.top_min, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->top_max, f.top_max, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
  }
  {
    const hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      bs_solids_free(out);
      return fail(ctx, BS_ERR_HIP, "hipStreamSynchronize (solids)", e);
    }
  }
  int64_t nv = 0, nf = 0, npx = 0, nw = 0, ncr = 0, vol = 0;
  for (int32_t c = 0; c < nb; c++) {
    nv += out->vertices[c];
    nf += out->faces[c];
    npx += out->pixels[c];
    nw += out->wall_faces[c];
    ncr += out->crossing_walls[c];
    vol += out->volume6[c];
  }
  const int64_t ni = (int64_t)tot[0];
  if (nv >= (1ll << 31) || ni >= (1ll << 31)) {
    bs_solids_free(out);
    return fail(ctx, BS_ERR_RANGE, "solids: 2^31 vertices or indices, or more");
  }

  // ---- scans (the sums fit 32 bits: checked above) ----
  hipError_t e = hipEventRecord(ev.e[5], st);
  if (e == hipSuccess)
    e = cub_run(B[SD_TMP], scan_v);
  if (e == hipSuccess)
    e = cub_run(B[SD_TMP], scan_f);
  if (e == hipSuccess)
    e = cub_run(B[SD_TMP], scan_i);
  if (e == hipSuccess)
    e = hipEventRecord(ev.e[6], st);
  if (e == hipSuccess && d_top)
    e = hipMemcpyAsync(d_top, top, 16 * (size_t)npix, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st);
  if (e == hipSuccess)
    e = hipGetLastError();
  if (e != hipSuccess) {
    bs_solids_free(out);
    return fail(ctx, BS_ERR_HIP, "solids: scans", e);
  }
  out->n_buildings = nb;
  out->width = w;
  out->height = h;
  out->bin = bin;
  out->base_z = base_z;
  out->n_pixels = npx;
  out->n_vertices = nv;
  out->n_faces = nf;
  out->n_indices = ni;
  out->n_wall_faces = nw;
  out->n_crossing_walls = ncr;
  out->total_volume6 = vol;
  out->ms_tops = ev.ms(0, 1);
  out->ms_vertices = ev.ms(1, 2);
  out->ms_faces = ev.ms(2, 3);
  out->ms_figures = ev.ms(3, 4);
  out->ms_scans = ev.ms(5, 6);
  ctx->sd_w = w;
  ctx->sd_h = h;
  ctx->sd_bin = bin;
  ctx->sd_base = base_z;
  ctx->sd_bases = d_bases != nullptr;
  ctx->sd_nv = nv;
  ctx->sd_nf = nf;
  ctx->sd_ni = ni;
  ctx->sd_valid = true;
  return BS_OK;
}

extern "C" int bs_solids_emit_dev(bs_ctx* ctx, int32_t* d_vertex, int32_t* d_face_offset, int32_t* d_face_index,
                                  int32_t* d_face_building, uint8_t* d_face_kind)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!ctx->sd_valid)
    return fail(ctx, BS_ERR_INVALID, "solids: emit without a successful bs_solids_count_dev on this context");
  const int64_t nv = ctx->sd_nv, nf = ctx->sd_nf, ni = ctx->sd_ni;
  if (!d_face_offset || (nv > 0 && !d_vertex) || (nf > 0 && (!d_face_index || !d_face_building || !d_face_kind)))
    return fail(ctx, BS_ERR_INVALID, "solids: emit: null pointer");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int w = ctx->sd_w, h = ctx->sd_h;
  const int64_t npix = (int64_t)w * h, nc = (int64_t)(w + 1) * (h + 1);
  DevBuf* B = ctx->sd;
  // (bs_set_building_bases ends the validity of a count, so the table is still the count's)
  const Bases bases{ctx->sd_bases ? ctx->bases_dev.as<int32_t>() : nullptr, ctx->sd_base};
  Events<3> ev;
  for (int k = 0; k < 3; k++)
    BS_HIP(ctx, hipEventCreate(&ev.e[k]));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  if (nv > 0)
    vertex_emit_kernel<<<grid_of(nc), 256, 0, st>>>(B[SD_MAP].as<int32_t>(), B[SD_TOP].as<int32_t>(), w, h, ctx->sd_bin,
                                                    bases, B[SD_VOFF].as<int32_t>(), reinterpret_cast<int4*>(d_vertex));
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  const FaceOut o{d_face_offset, d_face_index, d_face_building, d_face_kind};
  face_emit_kernel<<<grid_of(npix), 256, 0, st>>>(B[SD_MAP].as<int32_t>(), B[SD_TOP].as<int4>(), w, h, bases,
                                                  B[SD_VOFF].as<int32_t>(), B[SD_FOFF].as<int32_t>(),
                                                  B[SD_IOFF].as<int32_t>(), (int32_t)nf, (int32_t)ni, o);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  ctx->sd_ms_emit[0] = ev.ms(0, 1);
  ctx->sd_ms_emit[1] = ev.ms(1, 2);
  return BS_OK;
}

extern "C" int bs_solids(bs_ctx* ctx, const int32_t* map, const int32_t* roof, int32_t width, int32_t height,
                         int32_t n_buildings, int32_t n_planes, const double* normal, const int32_t* center,
                         const int32_t* z_min, const int32_t* z_max, int32_t bin, int32_t base_z, const int32_t* flat,
                         int32_t* top, struct bs_solids* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->sd_valid = false;
  if (out)
    memset(out, 0, sizeof *out);
  if (!map || !roof || !out || bad_image(width, height))
    return fail(ctx, BS_ERR_INVALID, SOLIDS_INVALID);
  const size_t npix = (size_t)width * height;
  DevBuf* B = ctx->sd;
  Staging S(ctx);
  const int32_t* d_map = S.upload(B[SD_IN_MAP], map, npix);
  const int32_t* d_roof = S.upload(B[SD_IN_ROOF], roof, npix);
  if (!S.ok())
    return S.status();
  int rc = bs_solids_count_dev(ctx, d_map, d_roof, width, height, n_buildings, n_planes, normal, center, z_min, z_max, bin, base_z,
                               flat, nullptr, out);
  if (rc != BS_OK)
    return rc;
  FreeUnlessKept<struct bs_solids, bs_solids_free> guard{out};
  DevMesh mesh(out->n_vertices, out->n_faces, out->n_indices);
  mesh.place(S.room<char>(B[SD_OUT], mesh.bytes()));
  if (S.ok()) {
    rc = bs_solids_emit_dev(ctx, mesh.vertex, mesh.face_offset, mesh.face_index, mesh.face_building, mesh.face_kind);
    if (rc != BS_OK)
      return rc;
    if (!mesh.to_host(S, *out)) {
      ctx->sd_valid = false;
      return fail(ctx, BS_ERR_NOMEM, "solids: host allocation");
    }
    S.download(top, B[SD_TOP].as<int32_t>(), 4 * npix);
  }
  rc = S.finish();
  if (rc != BS_OK) {
    ctx->sd_valid = false;
    return rc;
  }
  out->ms_emit_vertices = ctx->sd_ms_emit[0];
  out->ms_emit_faces = ctx->sd_ms_emit[1];
  guard.keep = true;
  return BS_OK;
}

// The format is written down in include/bs_api.h.
extern "C" int bs_solids_write_obj(const int32_t* vertex, int64_t n_vertices, const int32_t* face_offset,
                                   const int32_t* face_index, const int32_t* face_building, int64_t n_faces,
                                   int32_t n_buildings, const int32_t* origin, const char* path)
{
  if (!path || !face_offset || n_vertices < 0 || n_faces < 0 || n_buildings < 0 || n_vertices >= (1ll << 31) ||
      n_faces >= (1ll << 31) || (n_vertices > 0 && !vertex) || (n_faces > 0 && (!face_index || !face_building)))
    return BS_ERR_INVALID;
  if (face_offset[0] != 0)
    return BS_ERR_INVALID;
  std::vector<int64_t> first((size_t)n_buildings + 1, 0);  // counting sort by building, stable
  for (int64_t f = 0; f < n_faces; f++) {
    if (face_building[f] < 0 || face_building[f] >= n_buildings || face_offset[f + 1] < face_offset[f])
      return BS_ERR_INVALID;
    for (int32_t k = face_offset[f]; k < face_offset[f + 1]; k++)
      if (face_index[k] < 0 || face_index[k] >= n_vertices)
        return BS_ERR_INVALID;
    first[(size_t)face_building[f] + 1]++;
  }
  int32_t used = 0;
  for (int32_t c = 0; c < n_buildings; c++) {
    used += first[(size_t)c + 1] > 0;
    first[(size_t)c + 1] += first[c];
  }
  std::vector<int32_t> order((size_t)n_faces);
  {
    std::vector<int64_t> at(first.begin(), first.end() - 1);
    for (int64_t f = 0; f < n_faces; f++)
      order[(size_t)at[face_building[f]]++] = (int32_t)f;
  }
  FILE* fo = fopen(path, "w");
  if (!fo)
    return BS_ERR_INVALID;
  const int64_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  fprintf(fo, "# solids: %d buildings, %lld vertices, %lld faces\n", (int)used, (long long)n_vertices, (long long)n_faces);
  for (int64_t v = 0; v < n_vertices; v++)
    fprintf(fo, "v %lld %lld %lld\n", (long long)(vertex[4 * v] + o[0]), (long long)(vertex[4 * v + 1] + o[1]),
            (long long)(vertex[4 * v + 2] + o[2]));
  for (int32_t c = 0; c < n_buildings; c++) {
    if (first[(size_t)c + 1] == first[c])
      continue;
    fprintf(fo, "o building_%d\n", (int)c);
    for (int64_t q = first[c]; q < first[(size_t)c + 1]; q++) {
      const int32_t f = order[(size_t)q];
      fputc('f', fo);
      for (int32_t k = face_offset[f]; k < face_offset[f + 1]; k++)
        fprintf(fo, " %lld", (long long)face_index[k] + 1);
      fputc('\n', fo);
    }
  }
  const bool ok = !ferror(fo);
  return (fclose(fo) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}
