// bs_facet_dev.h -- the device passes of the roof facets (bs_facet.hip), shared with the roof generalisation
// (bs_generalise.hip), which runs them once per evaluation on its own scratch: label (tiles, seams, flatten), number,
// per-facet figures and border flags, border-edge keys, and the per-edge figures.  What each pass does is written down at
// the head of bs_facet.hip.
#pragma once

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>

#include "bs_common.h"
#include "bs_host.h"
#include "bs_segscan.h"
#include "bs_uf.h"

namespace bs {
namespace {

constexpr int LABEL_TW = 64, LABEL_TH = 16;  // labelling tile: a row is one wave, 8 KB (classes) + 4 KB (parents) of LDS
constexpr int GRID_CAP = 4096;   // workgroups of the grid-stride passes

inline int grid_of(int64_t n) { return (int)std::min<int64_t>(nblk(n, 256), GRID_CAP); }

constexpr unsigned long long NONE = ~0ull;  // the class of a pixel outside every building

// class of a pixel: (building << 32) | plane, plane 0 = unroofed
struct Cls {
  const int32_t* map;
  const int32_t* roof;
  __device__ unsigned long long operator()(int64_t i) const
  {
    const int32_t c = map[i];
    if (c < 0)
      return NONE;
    const int32_t r = roof[i];
    return ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(r > 0 ? r : 0);
  }
};

__device__ inline int lds_find(const volatile int* p, int x)
{
  int q;
  while ((q = p[x]) != x)
    x = q;
  return x;
}

// hook the larger root under the smaller one; atomicMin keeps parent <= self under races
__device__ inline void lds_union(int* p, int a, int b)
{
  for (;;) {
    a = lds_find(p, a);
    b = lds_find(p, b);
    if (a == b)
      return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(p + a, b);
    if (old == a)
      return;
    a = old;  // a was hooked elsewhere in the meantime: unite that root with b
  }
}

// ---- label ---------------------------------------------------------------------------------------------------------------
// One workgroup per tile.  A pixel joins W through its run, and N unless W and NW already carry the link.
__global__ __launch_bounds__(256) void facet_tile_kernel(Cls cls, int w, int h, int ntx, int32_t nb, int32_t npl,
                                                         int32_t* __restrict__ parent, int* __restrict__ bad)
{
  __shared__ unsigned long long c[LABEL_TH][LABEL_TW];
  __shared__ int p[LABEL_TH * LABEL_TW];
  const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int by = blockIdx.x / ntx, bx = blockIdx.x - by * ntx;
  const int x0 = bx * LABEL_TW, y0 = by * LABEL_TH, gx = x0 + lx;
  for (int j = 0; j < LABEL_TH / 4; j++) {
    const int ly = wv + 4 * j, gy = y0 + ly;
    unsigned long long v = NONE;
    if (gx < w && gy < h) {
      const int64_t i = (int64_t)gy * w + gx;
      const int32_t m = cls.map[i], r = cls.roof[i];
      if (m >= nb || r > npl || (r > 0 && m < 0))
        atomicOr(bad, 1);
      v = cls(i);
    }
    const unsigned long long left = __shfl_up(v, 1);
    const unsigned long long heads = __ballot(lx == 0 || v != left);
    c[ly][lx] = v;
    p[ly * LABEL_TW + lx] = ly * LABEL_TW + (v == NONE ? lx : head_lane(heads, lx));
  }
  __syncthreads();
  for (int j = 0; j < LABEL_TH / 4; j++) {
    const int ly = wv + 4 * j;
    const unsigned long long v = c[ly][lx];
    if (ly == 0 || v == NONE || c[ly - 1][lx] != v)
      continue;
    if (lx > 0 && c[ly][lx - 1] == v && c[ly - 1][lx - 1] == v)
      continue;
    lds_union(p, ly * LABEL_TW + lx, (ly - 1) * LABEL_TW + lx);
  }
  __syncthreads();
  for (int j = 0; j < LABEL_TH / 4; j++) {
    const int ly = wv + 4 * j, gy = y0 + ly;
    if (gx >= w || gy >= h)
      continue;
    int32_t out = -1;
    if (c[ly][lx] != NONE) {
      const int r = lds_find(p, ly * LABEL_TW + lx);
      out = (y0 + r / LABEL_TW) * w + x0 + (r & (LABEL_TW - 1));
    }
    parent[(int64_t)gy * w + gx] = out;
  }
}

// The links that cross a tile edge.  Threads [0, n_h) walk the rows y = LABEL_TH * k (k >= 1) and link north, the others the
// columns x = LABEL_TW * k (k >= 1) and link west.
__global__ __launch_bounds__(256) void facet_seam_kernel(Cls cls, int w, int h, int64_t n_h, int64_t total, int32_t* parent)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= total)
    return;
  int x, y;
  int32_t other;
  if (t < n_h) {
    const int64_t r = t / w;
    y = LABEL_TH * (int)(r + 1);
    x = (int)(t - r * w);
    other = (y - 1) * w + x;
  } else {
    const int64_t u = t - n_h;
    const int col = (int)(u / h);
    y = (int)(u - (int64_t)col * h);
    x = LABEL_TW * (col + 1);
    other = y * w + x - 1;
  }
  const int32_t i = y * w + x;
  const unsigned long long v = cls(i);
  if (v != NONE && cls(other) == v)
    uf_union(parent, i, other);
}

__global__ __launch_bounds__(256) void facet_flatten_kernel(int32_t* parent, int64_t np)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= np)
    return;
  int32_t p = parent[i];
  if (p < 0)
    return;
  int32_t r = (int32_t)i;
  while (p != r) {
    r = p;
    p = parent[r];
  }
  parent[i] = r;  // (racing writers store the same root; a stale read is still an ancestor)
}

// ---- number --------------------------------------------------------------------------------------------------------------
struct RootFlag {  // start pixel of a facet: a building pixel that is its own root
  const int32_t* parent;
  __host__ __device__ int32_t operator()(int32_t i) const { return parent[i] == i; }
};

__global__ __launch_bounds__(256) void facet_write_kernel(const int32_t* __restrict__ parent, const int32_t* __restrict__ scan,
                                                          int64_t np, int32_t* __restrict__ facet)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= np)
    return;
  const int32_t r = parent[i];
  facet[i] = r < 0 ? -1 : scan[r];
}

// ---- figures -------------------------------------------------------------------------------------------------------------
struct FacetFig {  // per facet, device
  unsigned long long* pixels;
  unsigned long long* inner;
  unsigned long long* outer;
  unsigned long long* top_sum;  // (two's complement sums)
  int32_t* bbox;
  int32_t* top_min;
  int32_t* top_max;
  int32_t* building;
  int32_t* plane;
  int32_t* start_xy;
};

FacetFig facet_fig_at(void* base, size_t n)
{
  FacetFig f;
  f.pixels = (unsigned long long*)base;
  f.inner = f.pixels + n;
  f.outer = f.inner + n;
  f.top_sum = f.outer + n;
  f.bbox = (int32_t*)(f.top_sum + n);
  f.top_min = f.bbox + 4 * n;
  f.top_max = f.top_min + n;
  f.building = f.top_max + n;
  f.plane = f.building + n;
  f.start_xy = f.plane + n;
  return f;
}
constexpr size_t FACET_FIG_BYTES = 4 * 8 + 10 * 4;

__global__ __launch_bounds__(256) void facet_fig_init_kernel(FacetFig f, int64_t nf)
{
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= nf)
    return;
  f.pixels[k] = f.inner[k] = f.outer[k] = f.top_sum[k] = 0;
  f.bbox[4 * k] = f.bbox[4 * k + 1] = INT32_MAX;
  f.bbox[4 * k + 2] = f.bbox[4 * k + 3] = INT32_MIN;
  f.top_min[k] = INT32_MAX;
  f.top_max[k] = INT32_MIN;
}

// Sides, border flags and per-facet figures of every pixel.  flags: bit 0 = the edge to (x + 1, y) is a border edge,
// bit 1 = the edge to (x, y + 1).
__global__ __launch_bounds__(256) void facet_figures_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ roof,
                                                            const int4* __restrict__ top, const int32_t* __restrict__ parent,
                                                            const int32_t* __restrict__ facet, int w, int h,
                                                            uint8_t* __restrict__ flags, FacetFig F)
{
  const int lane = threadIdx.x & 63;
  const int64_t npix = (int64_t)w * h, npix64 = (npix + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix64; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t f = -1, c = -1;
    int x = 0, y = 0;
    unsigned sides = 0;  // inner | outer << 16
    int32_t tmn = INT32_MAX, tmx = INT32_MIN;
    long long tsum = 0;
    if (i < npix) {
      c = map[i];
      unsigned fl = 0;
      if (c >= 0) {
        f = facet[i];
        y = (int)(i / w);
        x = (int)(i - (int64_t)y * w);
        const int4 T = top[i];
        tmn = min(min(T.x, T.y), min(T.z, T.w));
        tmx = max(max(T.x, T.y), max(T.z, T.w));
        tsum = (long long)T.x + T.y + T.z + T.w;
        // west, north, east, south: outer unless the neighbour is a pixel of the same building
        const bool sw = x > 0 && map[i - 1] == c, sn = y > 0 && map[i - w] == c;
        const bool se = x + 1 < w && map[i + 1] == c, ss = y + 1 < h && map[i + w] == c;
        const bool b_e = se && facet[i + 1] != f, b_s = ss && facet[i + w] != f;
        const unsigned inner = (unsigned)(sw && facet[i - 1] != f) + (unsigned)(sn && facet[i - w] != f) + b_e + b_s;
        const unsigned outer = 4u - (unsigned)sw - (unsigned)sn - (unsigned)se - (unsigned)ss;
        sides = inner | (outer << 16);
        fl = (unsigned)b_e | ((unsigned)b_s << 1);
        if (parent[i] == (int32_t)i) {  // the start pixel names the facet
          const int32_t r = roof[i];
          F.building[f] = c;
          F.plane[f] = r > 0 ? r : 0;
          F.start_xy[2 * f] = x;
          F.start_xy[2 * f + 1] = y;
        }
      }
      flags[i] = (uint8_t)fl;
    }
    const int32_t prev = __shfl_up(f, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != f);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    int xmn = x, xmx = x, ymn = y;
    BS_SEG_SCAN(sides, BS_OP_ADD)
    BS_SEG_SCAN(tsum, BS_OP_ADD)
    BS_SEG_SCAN(tmn, BS_OP_MIN)
    BS_SEG_SCAN(tmx, BS_OP_MAX)
    BS_SEG_SCAN(xmn, BS_OP_MIN)
    BS_SEG_SCAN(xmx, BS_OP_MAX)
    BS_SEG_SCAN(ymn, BS_OP_MIN)
    if (lane == tl && f >= 0) {  // (y ascends along a run: this lane holds its largest)
      atomicAdd(F.pixels + f, (unsigned long long)(tl - hl + 1));
      if (sides & 0xFFFFu)
        atomicAdd(F.inner + f, (unsigned long long)(sides & 0xFFFFu));
      if (sides >> 16)
        atomicAdd(F.outer + f, (unsigned long long)(sides >> 16));
      atomicAdd(F.top_sum + f, (unsigned long long)tsum);
      atomicMin(F.top_min + f, tmn);
      atomicMax(F.top_max + f, tmx);
      atomicMin(F.bbox + 4 * (int64_t)f, xmn);
      atomicMin(F.bbox + 4 * (int64_t)f + 1, ymn);
      atomicMax(F.bbox + 4 * (int64_t)f + 2, xmx);
      atomicMax(F.bbox + 4 * (int64_t)f + 3, y);
    }
  }
}

// ---- edges ---------------------------------------------------------------------------------------------------------------
struct FlagCount {
  __host__ __device__ int32_t operator()(uint8_t v) const { return (v & 1) + (v >> 1); }
};
using FlagIt = hipcub::TransformInputIterator<int32_t, FlagCount, const uint8_t*>;

__global__ __launch_bounds__(256) void edge_emit_kernel(const uint8_t* __restrict__ flags, const int32_t* __restrict__ eoff,
                                                        const int32_t* __restrict__ facet, int w, int64_t npix,
                                                        unsigned long long* __restrict__ keys, int32_t* __restrict__ vals)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned fl = flags[i];
    if (!fl)
      continue;
    const unsigned fa = (unsigned)facet[i];
    int32_t at = eoff[i];
    if (fl & 1u) {
      const unsigned fb = (unsigned)facet[i + 1];
      keys[at] = ((unsigned long long)min(fa, fb) << 32) | max(fa, fb);
      vals[at] = (int32_t)(2 * i);
      at++;
    }
    if (fl & 2u) {
      const unsigned fb = (unsigned)facet[i + w];
      keys[at] = ((unsigned long long)min(fa, fb) << 32) | max(fa, fb);
      vals[at] = (int32_t)(2 * i + 1);
    }
  }
}

struct HeadFlag {  // first sorted item of an edge
  const unsigned long long* keys;
  __host__ __device__ int32_t operator()(int32_t j) const { return j == 0 || keys[j] != keys[j - 1]; }
};

struct EdgeFig {  // per edge, device
  unsigned long long* length;
  unsigned long long* n_dir0;
  unsigned long long* n_step;
  unsigned long long* step_abs_sum;
  unsigned long long* step_abs_max;
  unsigned long long* rise_sum;  // (two's complement sums)
  unsigned long long* bend_sum;
  int32_t* facet;
  int32_t* building;
  int32_t* z_min;
  int32_t* z_max;
  int32_t* bbox;
};

EdgeFig edge_fig_at(void* base, size_t n)
{
  EdgeFig f;
  f.length = (unsigned long long*)base;
  f.n_dir0 = f.length + n;
  f.n_step = f.n_dir0 + n;
  f.step_abs_sum = f.n_step + n;
  f.step_abs_max = f.step_abs_sum + n;
  f.rise_sum = f.step_abs_max + n;
  f.bend_sum = f.rise_sum + n;
  f.facet = (int32_t*)(f.bend_sum + n);
  f.building = f.facet + 2 * n;
  f.z_min = f.building + n;
  f.z_max = f.z_min + n;
  f.bbox = f.z_max + n;
  return f;
}
constexpr size_t EDGE_FIG_BYTES = 7 * 8 + 9 * 4;

__global__ __launch_bounds__(256) void edge_fig_init_kernel(EdgeFig f, int64_t ne)
{
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= ne)
    return;
  f.length[k] = f.n_dir0[k] = f.n_step[k] = f.step_abs_sum[k] = f.step_abs_max[k] = f.rise_sum[k] = f.bend_sum[k] = 0;
  f.z_min[k] = INT32_MAX;
  f.z_max[k] = INT32_MIN;
  f.bbox[4 * k] = f.bbox[4 * k + 1] = INT32_MAX;
  f.bbox[4 * k + 2] = f.bbox[4 * k + 3] = INT32_MIN;
}

// One lane per sorted border edge: its figures from top by the pixel-edge number, reduced over the runs of equal edge
// inside the wave, one set of atomics per run.  eid is the INCLUSIVE sum of the run heads: edge = eid - 1.
__global__ __launch_bounds__(256) void edge_reduce_kernel(const unsigned long long* __restrict__ keys,
                                                          const int32_t* __restrict__ vals, const int32_t* __restrict__ eid,
                                                          int64_t nbord, const int32_t* __restrict__ map,
                                                          const int4* __restrict__ top, const int32_t* __restrict__ facet,
                                                          int w, EdgeFig E)
{
  const int lane = threadIdx.x & 63;
  const int64_t n64 = (nbord + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n64; j += (int64_t)gridDim.x * blockDim.x) {
    int32_t e = -1;
    bool dir0 = false, step = false;
    long long asum = 0, amax = 0, rise = 0, bend = 0;
    int32_t zmn = INT32_MAX, zmx = INT32_MIN;
    int X0 = INT32_MAX, Y0 = INT32_MAX, X1 = INT32_MIN, Y1 = INT32_MIN;
    if (j < nbord) {
      e = eid[j] - 1;
      const int32_t v = vals[j];
      const int64_t a = v >> 1;
      const int d = v & 1;
      const int64_t b = a + (d ? w : 1);
      const int y = (int)(a / w), x = (int)(a - (int64_t)y * w);
      const int4 A = top[a], B = top[b];
      // the tops at the shared corners s and e, and the rise of each pixel across the edge
      const long long a_s = d ? A.z : A.y, a_e = A.w, b_s = B.x, b_e = d ? B.y : B.z;
      const long long sa = d ? ((long long)A.z + A.w) - ((long long)A.x + A.y) : ((long long)A.y + A.w) - ((long long)A.x + A.z);
      const long long sb = d ? ((long long)B.z + B.w) - ((long long)B.x + B.y) : ((long long)B.y + B.w) - ((long long)B.x + B.z);
      const long long ds = a_s - b_s, de = a_e - b_e;
      dir0 = d == 0;
      step = ds != 0 || de != 0;
      const long long as_abs = ds < 0 ? -ds : ds, ae_abs = de < 0 ? -de : de;
      asum = as_abs + ae_abs;
      amax = as_abs > ae_abs ? as_abs : ae_abs;
      rise = facet[a] > facet[b] ? ds + de : -(ds + de);
      bend = sa - sb;
      zmn = (int32_t)min(min(a_s, a_e), min(b_s, b_e));
      zmx = (int32_t)max(max(a_s, a_e), max(b_s, b_e));
      X0 = d ? x : x + 1;
      Y0 = d ? y + 1 : y;
      X1 = x + 1;
      Y1 = y + 1;
      const int32_t before = j == 0 ? 0 : eid[j - 1];
      if (before != e + 1) {  // the first item of the edge names it
        const unsigned long long k = keys[j];
        E.facet[2 * (int64_t)e] = (int32_t)(k >> 32);
        E.facet[2 * (int64_t)e + 1] = (int32_t)(k & 0xFFFFFFFFull);
        E.building[e] = map[a];
      }
    }
    const int32_t prev = __shfl_up(e, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != e);
    const unsigned long long m_dir0 = __ballot(dir0), m_step = __ballot(step);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    BS_SEG_SCAN(asum, BS_OP_ADD)
    BS_SEG_SCAN(amax, BS_OP_MAX)
    BS_SEG_SCAN(rise, BS_OP_ADD)
    BS_SEG_SCAN(bend, BS_OP_ADD)
    BS_SEG_SCAN(zmn, BS_OP_MIN)
    BS_SEG_SCAN(zmx, BS_OP_MAX)
    BS_SEG_SCAN(X0, BS_OP_MIN)
    BS_SEG_SCAN(Y0, BS_OP_MIN)
    BS_SEG_SCAN(X1, BS_OP_MAX)
    BS_SEG_SCAN(Y1, BS_OP_MAX)
    if (lane == tl && e >= 0) {
      const int len = tl - hl + 1;
      const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1)) << hl;
      const unsigned nd0 = (unsigned)__popcll(m_dir0 & run), nst = (unsigned)__popcll(m_step & run);
      atomicAdd(E.length + e, (unsigned long long)len);
      if (nd0)
        atomicAdd(E.n_dir0 + e, (unsigned long long)nd0);
      if (nst) {
        atomicAdd(E.n_step + e, (unsigned long long)nst);
        atomicAdd(E.step_abs_sum + e, (unsigned long long)asum);
        atomicMax(E.step_abs_max + e, (unsigned long long)amax);
        atomicAdd(E.rise_sum + e, (unsigned long long)rise);
      }
      atomicAdd(E.bend_sum + e, (unsigned long long)bend);
      atomicMin(E.z_min + e, zmn);
      atomicMax(E.z_max + e, zmx);
      atomicMin(E.bbox + 4 * (int64_t)e, X0);
      atomicMin(E.bbox + 4 * (int64_t)e + 1, Y0);
      atomicMax(E.bbox + 4 * (int64_t)e + 2, X1);
      atomicMax(E.bbox + 4 * (int64_t)e + 3, Y1);
    }
  }
}

}  // namespace
}  // namespace bs
