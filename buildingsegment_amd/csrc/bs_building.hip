// bs_building.hip -- which points and which planes belong to which building footprint ("Buildings").
//   1. label   union-find over the padded (W+2) x (H+2) grid in two levels: one workgroup per TW x TH tile unites
//              tile-local indices in LDS (a row of a tile is one wave: horizontal runs come from a ballot, only the
//              vertical and diagonal links go through LDS atomics) and writes every pixel the GLOBAL index of its
//              tile-component's first pixel; a seam kernel unites across tile edges with bs_uf.h; one flatten pass.
//              parent <= self throughout, so a root is its component's first raster pixel.  Run twice, the class of a
//              pixel being a template parameter: pass 1 foreground (8-connected) / background (4-connected), pass 2
//              "not outer background" (8-connected) / outer background.
//   2. number  roots of pass 2 flagged and scanned; building c = (number of roots) - 1 - rank, i.e. descending start
//              pixel = the contour order of bs_footprints; the unpadded int32 map and the pixel figures of every
//              building (per run of equal pixels inside a wave, through LDS tables for buildings < FIG_CAP)
//   3. assign  one thread per point: map look-up at the base pixel of its splat, figures reduced in the wave (all
//              lanes in one building) or in LDS tables (building < FIG_CAP) before one global atomic per
//              (workgroup, building, figure); buildings >= FIG_CAP go straight to global atomics
//   4. votes   exact (plane, building) counts: a dense histogram (workgroup-private in LDS when it fits), or a radix
//              sort of the keys + run lengths; per-plane arg-max by an atomicMax on (count, ~building)
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bs_common.h"
#include "bs_host.h"
#include "bs_uf.h"

namespace bs {
namespace {

constexpr int TW = 64, TH = 16;           // labelling tile: a row is one wave, 4 KB + 1 KB of LDS
constexpr int FIG_CAP = 256;              // buildings whose pixel and point figures are reduced in LDS (6 KB)
constexpr int VOTE_LDS_CELLS = 8192;      // dense vote histogram kept per workgroup in LDS (32 KB)
constexpr int64_t VOTE_DENSE_CELLS = 1ll << 22;  // dense vote histogram in HBM (16 MB); above: sort + run lengths
// scratch of bs_ctx::bd
enum { BD_LAB1, BD_LAB2, BD_SCAN, BD_TMP, BD_PIX, BD_MISC, BD_FIG, BD_VOTE, BD_KEYS, BD_KEYS2, BD_RUNS, BD_IN_A, BD_IN_B,
       BD_IN_C };

// ---- classes of the two labelling passes: 1 = the 8-connected class, 0 = the 4-connected one ---------------------
struct MaskClass {  // pass 1 on the unpadded mask: foreground / background (the frame is background)
  const uint8_t* m;
  int w, h;
  __device__ int operator()(int x, int y) const
  {
    return x >= 1 && x <= w && y >= 1 && y <= h && m[(int64_t)(y - 1) * w + (x - 1)] != 0;
  }
};
struct FilledClass {  // pass 2 on the labels of pass 1: everything but the frame's background component (root 0)
  const int32_t* lab;
  int wp;
  __device__ int operator()(int x, int y) const { return lab[(int64_t)y * wp + x] != 0; }
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

// One workgroup per tile.  A pixel joins W always (runs), N unless W and NW already carry the link, and for class 1
// NW / NE where N does not carry it -- cc_union_kernel's set restricted to neighbours inside the tile.
template <class Cls>
__global__ __launch_bounds__(256) void label_tile_kernel(Cls cls, int wp, int hp, int ntx, int32_t* __restrict__ parent)
{
  __shared__ uint8_t c[TH][TW];  // 0 / 1; 2 = outside the grid
  __shared__ int p[TH * TW];
  const int lx = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int by = blockIdx.x / ntx, bx = blockIdx.x - by * ntx;
  const int x0 = bx * TW, y0 = by * TH, gx = x0 + lx;
  for (int j = 0; j < TH / 4; j++) {
    const int ly = wv + 4 * j, gy = y0 + ly;
    const int v = (gx < wp && gy < hp) ? cls(gx, gy) : 2;
    const unsigned long long m1 = __ballot(v == 1), m0 = __ballot(v == 0);
    const unsigned long long other = ~(v == 1 ? m1 : m0) & ((1ull << lx) - 1);  // lanes left of me outside my run
    const int start = v == 2 ? lx : (other ? 64 - __clzll(other) : 0);
    c[ly][lx] = (uint8_t)v;
    p[ly * TW + lx] = ly * TW + start;
  }
  __syncthreads();
  for (int j = 0; j < TH / 4; j++) {
    const int ly = wv + 4 * j;
    const int v = c[ly][lx];
    if (ly == 0 || v == 2)
      continue;
    const int i = ly * TW + lx;
    const int n = c[ly - 1][lx];
    const int nw = lx > 0 ? c[ly - 1][lx - 1] : 2;
    const bool w_same = lx > 0 && c[ly][lx - 1] == v;
    if (n == v && !(w_same && nw == v))
      lds_union(p, i, i - TW);
    if (v == 1 && n != 1) {
      if (nw == 1 && !w_same)
        lds_union(p, i, i - TW - 1);
      if (lx < TW - 1 && c[ly - 1][lx + 1] == 1)
        lds_union(p, i, i - TW + 1);
    }
  }
  __syncthreads();
  for (int j = 0; j < TH / 4; j++) {
    const int ly = wv + 4 * j, gy = y0 + ly;
    if (gx >= wp || gy >= hp)
      continue;
    const int r = lds_find(p, ly * TW + lx);
    parent[(int64_t)gy * wp + gx] = (y0 + r / TW) * wp + x0 + (r & (TW - 1));
  }
}

// The links of cc_union_kernel's set that cross a tile edge.  Threads [0, n_h) walk the rows y = TH * k (k >= 1),
// the others the columns x = TW * k and TW * k - 1 (k >= 1) outside those rows.  NW / NE only for class 1.
template <class Cls>
__global__ __launch_bounds__(256) void label_seam_kernel(Cls cls, int wp, int hp, int64_t n_h, int64_t total,
                                                         int32_t* parent)
{
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= total)
    return;
  int x, y;
  if (t < n_h) {
    const int64_t r = t / wp;
    y = TH * (int)(r + 1);
    x = (int)(t - r * wp);
  } else {
    const int64_t u = t - n_h;
    const int col = (int)(u / hp);
    y = (int)(u - (int64_t)col * hp);
    if (y > 0 && y % TH == 0)
      return;
    x = TW * (col / 2 + 1) - (col & 1);
  }
  const int v = cls(x, y);
  const int32_t i = y * wp + x;
  const bool cross_w = x % TW == 0, cross_n = y % TH == 0, cross_e = x % TW == TW - 1;
  const bool w_same = x > 0 && cls(x - 1, y) == v;
  if (w_same && cross_w)
    uf_union(parent, i, i - 1);
  if (y == 0)
    return;
  const int n = cls(x, y - 1);
  const int nw = x > 0 ? cls(x - 1, y - 1) : 2;
  if (cross_n && n == v && !(w_same && nw == v))
    uf_union(parent, i, i - wp);
  if (v == 1 && n != 1) {
    if ((cross_n || cross_w) && nw == 1 && !w_same)
      uf_union(parent, i, i - wp - 1);
    if ((cross_n || cross_e) && x < wp - 1 && cls(x + 1, y - 1) == 1)
      uf_union(parent, i, i - wp + 1);
  }
}

__global__ __launch_bounds__(256) void label_flatten_kernel(int32_t* parent, int64_t np)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= np)
    return;
  int32_t r = (int32_t)i, p = parent[r];
  while (p != r) {
    r = p;
    p = parent[r];
  }
  parent[i] = r;  // (racing writers store the same root; a stale read is still an ancestor)
}

// start pixel of a building: a filled pixel that is its own root in pass 2
struct RootFlag {
  const int32_t* lab1;
  const int32_t* lab2;
  __host__ __device__ int32_t operator()(int32_t i) const { return lab1[i] != 0 && lab2[i] == i; }
};

struct PixFig {  // per building, device
  int32_t* start_xy;
  int32_t* bbox;
  unsigned long long* pixels;
  unsigned long long* fg;
};

__global__ __launch_bounds__(256) void pixfig_init_kernel(PixFig f, int32_t nb)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb)
    return;
  f.bbox[4 * c] = f.bbox[4 * c + 1] = INT32_MAX;
  f.bbox[4 * c + 2] = f.bbox[4 * c + 3] = INT32_MIN;
  f.pixels[c] = f.fg[c] = 0;
}

// map[y][x] = nb - 1 - rank(root) or -1.  The figures leave a wave once per run of equal buildings inside its 64
// consecutive pixels of one row; runs of buildings < FIG_CAP meet in LDS tables first (a one-pixel spiral has millions
// of runs of ONE building), so that HBM sees one atomic per (workgroup, building, figure); the others go straight
// to global atomics
__device__ inline void pixfig_global(const PixFig& f, int32_t b, unsigned pix, unsigned nfg, int x0, int y0, int x1, int y1)
{
  atomicAdd(f.pixels + b, (unsigned long long)pix);
  if (nfg)
    atomicAdd(f.fg + b, (unsigned long long)nfg);
  atomicMin(f.bbox + 4 * b, x0);
  atomicMin(f.bbox + 4 * b + 1, y0);
  atomicMax(f.bbox + 4 * b + 2, x1);
  atomicMax(f.bbox + 4 * b + 3, y1);
}

__global__ __launch_bounds__(256) void map_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ lab1,
                                                  const int32_t* __restrict__ lab2, const int32_t* __restrict__ scan,
                                                  int w, int h, int32_t nb, int32_t* __restrict__ map, PixFig f)
{
  __shared__ unsigned s_pix[FIG_CAP], s_fg[FIG_CAP];
  __shared__ int s_x0[FIG_CAP], s_y0[FIG_CAP], s_x1[FIG_CAP], s_y1[FIG_CAP];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    s_pix[k] = s_fg[k] = 0;
    s_x0[k] = s_y0[k] = INT32_MAX;
    s_x1[k] = s_y1[k] = INT32_MIN;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wp = w + 2;
  const int64_t npix = (int64_t)w * h;
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < npix; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    int32_t b = -1;
    int x = 0, y = 0;
    bool fg = false;
    if (i < npix) {
      y = (int)(i / w);
      x = (int)(i - (int64_t)y * w);
      const int32_t pi = (y + 1) * wp + x + 1;
      if (lab1[pi] != 0) {
        const int32_t r = lab2[pi];
        b = nb - 1 - scan[r];
        fg = mask[i] != 0;
        if (r == pi) {
          f.start_xy[2 * b] = x;
          f.start_xy[2 * b + 1] = y;
        }
      }
      map[i] = b;
    }
    const int32_t prev = __shfl_up(b, 1);
    const bool head = lane == 0 || prev != b || x == 0;
    const unsigned long long heads = __ballot(head), fgm = __ballot(fg);
    if (head && b >= 0) {
      const unsigned long long above = lane == 63 ? 0 : heads & (~0ull << (lane + 1));
      const int end = above ? __ffsll((long long)above) - 1 : 64;  // one past the run's last lane
      const int len = end - lane;
      const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1)) << lane;
      const unsigned nfg = (unsigned)__popcll(fgm & run);
      if (b < FIG_CAP) {
        atomicAdd(s_pix + b, (unsigned)len);
        if (nfg)
          atomicAdd(s_fg + b, nfg);
        atomicMin(s_x0 + b, x);
        atomicMin(s_y0 + b, y);
        atomicMax(s_x1 + b, x + len - 1);
        atomicMax(s_y1 + b, y);
      } else {
        pixfig_global(f, b, (unsigned)len, nfg, x, y, x + len - 1, y);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x)
    if (s_pix[k])
      pixfig_global(f, k, s_pix[k], s_fg[k], s_x0[k], s_y0[k], s_x1[k], s_y1[k]);
}

// ---- points ------------------------------------------------------------------------------------------------------
struct PtFig {  // per building, device
  unsigned long long* n_points;
  unsigned long long* n_above;
  int32_t* z_min;
  int32_t* z_max;
  unsigned long long* z_sum;
};

__global__ __launch_bounds__(256) void ptfig_init_kernel(PtFig f, int32_t nb)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb)
    return;
  f.n_points[c] = f.n_above[c] = f.z_sum[c] = 0;
  f.z_min[c] = INT32_MAX;
  f.z_max[c] = INT32_MIN;
}

__device__ inline void fig_global(const PtFig& f, int32_t b, unsigned cnt, unsigned abv, int32_t zmn, int32_t zmx,
                                  unsigned long long zs)
{
  atomicAdd(f.n_points + b, (unsigned long long)cnt);
  if (abv) {
    atomicAdd(f.n_above + b, (unsigned long long)abv);
    atomicMin(f.z_min + b, zmn);
    atomicMax(f.z_max + b, zmx);
    atomicAdd(f.z_sum + b, zs);
  }
}

__global__ __launch_bounds__(256) void assign_kernel(const int32_t* __restrict__ xyz, int64_t n, int bin, double ground_th,
                                                     GroundRule rule,
                                                     const int32_t* __restrict__ map, int w, int h, int32_t nb,
                                                     int32_t* __restrict__ bidx, PtFig f, int* __restrict__ bad)
{
  __shared__ unsigned s_cnt[FIG_CAP], s_abv[FIG_CAP];
  __shared__ int s_mn[FIG_CAP], s_mx[FIG_CAP];
  __shared__ unsigned long long s_sum[FIG_CAP];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    s_cnt[k] = s_abv[k] = 0;
    s_mn[k] = INT32_MAX;
    s_mx[k] = INT32_MIN;
    s_sum[k] = 0;
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, n64 = (n + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n64; i += stride) {
    int32_t b = -1, x = 0, y = 0, z = 0;
    if (i < n) {
      x = xyz[3 * i];
      y = xyz[3 * i + 1];
      z = xyz[3 * i + 2];
      const int32_t px = x / bin, py = y / bin;  // base pixel of the splat, TMC3.cpp:134-135
      if (x < 0 || y < 0 || px >= w || py >= h)
        atomicOr(bad, 1);
      else
        b = map[(int64_t)py * w + px];
      if (b >= nb)
        b = -1;  // (a map of another struct: stay in bounds)
      bidx[i] = b;
    }
    const bool above = b >= 0 && !rule.below(x, y, z, ground_th);  // TMC3.cpp:139
    const int32_t b0 = __shfl(b, 0);
    if (__all(b == b0)) {  // the whole wave in one building (clouds in spatial order): reduce in registers
      if (b0 < 0)
        continue;
      const unsigned abv = (unsigned)__popcll(__ballot(above));
      int32_t mn = above ? z : INT32_MAX, mx = above ? z : INT32_MIN;
      unsigned long long zs = above ? (unsigned long long)(long long)z : 0;
      for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o));
        mx = max(mx, __shfl_xor(mx, o));
        zs += __shfl_xor(zs, o);
      }
      if ((threadIdx.x & 63) == 0) {
        if (b0 < FIG_CAP) {
          atomicAdd(s_cnt + b0, 64u);
          if (abv) {
            atomicAdd(s_abv + b0, abv);
            atomicMin(s_mn + b0, mn);
            atomicMax(s_mx + b0, mx);
            atomicAdd(s_sum + b0, zs);
          }
        } else {
          fig_global(f, b0, 64u, abv, mn, mx, zs);
        }
      }
    } else if (b >= 0) {
      if (b < FIG_CAP) {
        atomicAdd(s_cnt + b, 1u);
        if (above) {
          atomicAdd(s_abv + b, 1u);
          atomicMin(s_mn + b, z);
          atomicMax(s_mx + b, z);
          atomicAdd(s_sum + b, (unsigned long long)(long long)z);
        }
      } else {
        fig_global(f, b, 1u, above ? 1u : 0u, z, z, (unsigned long long)(long long)z);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x)
    if (s_cnt[k])
      fig_global(f, k, s_cnt[k], s_abv[k], s_mn[k], s_mx[k], s_sum[k]);
}

// ---- votes -------------------------------------------------------------------------------------------------------
// cell of a point: (plane - 1) * (nb + 1) + building + 1; -1: not a plane 1..n_planes; -2: building out of range
__device__ inline int64_t vote_cell(int32_t p, int32_t b, int32_t n_planes, int32_t nb)
{
  if (p < 1 || p > n_planes)
    return -1;
  if (b < -1 || b >= nb)
    return -2;
  return (int64_t)(p - 1) * (nb + 1) + (b + 1);
}

template <bool LDS>
__global__ __launch_bounds__(256) void vote_hist_kernel(const int32_t* __restrict__ plane, const int32_t* __restrict__ bidx,
                                                        int64_t n, int32_t n_planes, int32_t nb, int32_t cells,
                                                        unsigned* __restrict__ hist, int* __restrict__ bad)
{
  __shared__ unsigned s[LDS ? VOTE_LDS_CELLS : 1];
  if (LDS) {
    for (int k = threadIdx.x; k < cells; k += blockDim.x)
      s[k] = 0;
    __syncthreads();
  }
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = vote_cell(plane[i], bidx[i], n_planes, nb);
    if (c == -2)
      atomicOr(bad, 1);
    if (c < 0)
      continue;
    if (LDS)
      atomicAdd(s + c, 1u);
    else
      atomicAdd(hist + c, 1u);
  }
  if (LDS) {
    __syncthreads();
    for (int k = threadIdx.x; k < cells; k += blockDim.x)
      if (s[k])
        atomicAdd(hist + k, s[k]);
  }
}

struct Votes {  // per plane, device
  unsigned long long* total;
  unsigned long long* outside;
  unsigned long long* best;  // (count << 32) | ~building: the maximum is the largest count, then the lowest building
};

__device__ inline void vote(const Votes& v, int64_t cell, unsigned long long cnt, int32_t nb)
{
  if (!cnt)
    return;
  const int64_t p = cell / (nb + 1);
  const uint32_t col = (uint32_t)(cell - p * (nb + 1));
  atomicAdd(v.total + p, cnt);
  if (col == 0)
    v.outside[p] = cnt;  // (one cell, one run: a single writer)
  else
    atomicMax(v.best + p, (cnt << 32) | (0xFFFFFFFFu - (col - 1)));
}

__global__ __launch_bounds__(256) void vote_cells_kernel(const unsigned* __restrict__ hist, int64_t cells, int32_t nb, Votes v)
{
  const int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (c < cells)
    vote(v, c, hist[c], nb);
}

__global__ __launch_bounds__(256) void vote_keys_kernel(const int32_t* __restrict__ plane, const int32_t* __restrict__ bidx,
                                                        int64_t n, int32_t n_planes, int32_t nb, uint64_t none,
                                                        uint64_t* __restrict__ keys, int* __restrict__ bad)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int64_t c = vote_cell(plane[i], bidx[i], n_planes, nb);
  if (c == -2)
    atomicOr(bad, 1);
  keys[i] = c < 0 ? none : (uint64_t)c;
}

__global__ __launch_bounds__(256) void vote_runs_kernel(const uint64_t* __restrict__ key, const int32_t* __restrict__ len,
                                                        const int32_t* __restrict__ n_runs, uint64_t none, int32_t nb, Votes v)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r < *n_runs && key[r] != none)
    vote(v, (int64_t)key[r], (unsigned long long)len[r], nb);
}

template <class Cls>
void launch_label(Cls cls, int wp, int hp, int32_t* parent, hipStream_t st)
{
  const int ntx = nblk(wp, TW), nty = nblk(hp, TH);
  const int64_t np = (int64_t)wp * hp;
  label_tile_kernel<Cls><<<(unsigned)((int64_t)ntx * nty), 256, 0, st>>>(cls, wp, hp, ntx, parent);
  const int64_t n_h = (int64_t)(nty - 1) * wp, total = n_h + (int64_t)(ntx - 1) * 2 * hp;
  if (total > 0)
    label_seam_kernel<Cls><<<nblk(total, 256), 256, 0, st>>>(cls, wp, hp, n_h, total, parent);
  label_flatten_kernel<<<nblk(np, 256), 256, 0, st>>>(parent, np);
}

bool alloc_buildings(bs_buildings* b, int32_t nb)
{
  const size_t m = (size_t)std::max(nb, 1);
  b->start_xy = (int32_t*)calloc(2 * m, 4);
  b->bbox = (int32_t*)calloc(4 * m, 4);
  b->pixels = (int64_t*)calloc(m, 8);
  b->fg_pixels = (int64_t*)calloc(m, 8);
  b->n_points = (int64_t*)calloc(m, 8);
  b->n_above = (int64_t*)calloc(m, 8);
  b->z_min = (int32_t*)calloc(m, 4);
  b->z_max = (int32_t*)calloc(m, 4);
  b->z_sum = (int64_t*)calloc(m, 8);
  if (!b->start_xy || !b->bbox || !b->pixels || !b->fg_pixels || !b->n_points || !b->n_above || !b->z_min || !b->z_max ||
      !b->z_sum)
    return false;
  for (int32_t c = 0; c < nb; c++) {
    b->z_min[c] = INT32_MAX;
    b->z_max[c] = INT32_MIN;
  }
  return true;
}

bool bad_raster(int32_t w, int32_t h) { return w < 1 || h < 1 || (int64_t)(w + 2ll) * (h + 2ll) >= (1ll << 31); }

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_buildings_free(bs_buildings* b)
{
  if (!b)
    return;
  free(b->start_xy);
  free(b->bbox);
  free(b->pixels);
  free(b->fg_pixels);
  free(b->n_points);
  free(b->n_above);
  free(b->z_min);
  free(b->z_max);
  free(b->z_sum);
  memset(b, 0, sizeof *b);
}

extern "C" int bs_building_map_dev(bs_ctx* ctx, const uint8_t* d_mask, int32_t width, int32_t height, int32_t* d_map,
                                   bs_buildings* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (out)
    memset(out, 0, sizeof *out);
  if (!d_mask || !d_map || !out || bad_raster(width, height))
    return fail(ctx, BS_ERR_INVALID, "building map: null pointer or bad raster size");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int w = width, h = height, wp = w + 2, hp = h + 2;
  const int64_t np = (int64_t)wp * hp, npix = (int64_t)w * h;
  DevBuf* B = ctx->bd;
  Events<5> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));
  BS_HIP(ctx, B[BD_LAB1].reserve(4 * np));
  BS_HIP(ctx, B[BD_LAB2].reserve(4 * np));
  BS_HIP(ctx, B[BD_SCAN].reserve(4 * np));
  int32_t* lab1 = B[BD_LAB1].as<int32_t>();
  int32_t* lab2 = B[BD_LAB2].as<int32_t>();
  int32_t* scan = B[BD_SCAN].as<int32_t>();

  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  launch_label(MaskClass{d_mask, w, h}, wp, hp, lab1, st);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  launch_label(FilledClass{lab1, wp}, wp, hp, lab2, st);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));

  hipcub::CountingInputIterator<int32_t> idx(0);
  hipcub::TransformInputIterator<int32_t, RootFlag, hipcub::CountingInputIterator<int32_t>> flags(idx, RootFlag{lab1, lab2});
  BS_HIP(ctx, cub_run(B[BD_TMP], [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, flags, scan, (int)np, st);
  }));
  int32_t nb = 0;  // (the last padded pixel lies on the frame: never a start pixel)
  BS_HIP(ctx, hipMemcpyAsync(&nb, scan + np - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());

  const size_t m = (size_t)std::max(nb, 1);
  BS_HIP(ctx, B[BD_PIX].reserve(40 * m));
  PixFig f;
  f.pixels = B[BD_PIX].as<unsigned long long>();
  f.fg = f.pixels + m;
  f.start_xy = reinterpret_cast<int32_t*>(f.fg + m);
  f.bbox = f.start_xy + 2 * m;
  if (nb > 0)
    pixfig_init_kernel<<<nblk(nb, 256), 256, 0, st>>>(f, nb);
  map_kernel<<<(int)std::min<int64_t>(nblk(npix, 256), 4096), 256, 0, st>>>(d_mask, lab1, lab2, scan, w, h, nb, d_map, f);
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  if (!alloc_buildings(out, nb)) {
    bs_buildings_free(out);
    return fail(ctx, BS_ERR_NOMEM, "building map: host allocation");
  }
  if (nb > 0) {
    BS_HIP(ctx, hipMemcpyAsync(out->pixels, f.pixels, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->fg_pixels, f.fg, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->start_xy, f.start_xy, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->bbox, f.bbox, 16 * (size_t)nb, hipMemcpyDeviceToHost, st));
  }
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  out->n_buildings = nb;
  out->width = w;
  out->height = h;
  out->ms_label_mask = ev.ms(0, 1);
  out->ms_label_fill = ev.ms(1, 2);
  out->ms_number = ev.ms(2, 3);
  out->ms_map = ev.ms(3, 4);
  return BS_OK;
}

extern "C" int bs_building_map(bs_ctx* ctx, const uint8_t* mask, int32_t width, int32_t height, int32_t* map,
                               bs_buildings* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (out)
    memset(out, 0, sizeof *out);
  if (!mask || !map || !out || bad_raster(width, height))
    return fail(ctx, BS_ERR_INVALID, "building map: null pointer or bad raster size");
  const size_t npix = (size_t)width * height;
  Staging S(ctx);
  const uint8_t* d_mask = S.upload(ctx->bd[BD_IN_A], mask, npix);
  int32_t* d_map = S.room<int32_t>(ctx->bd[BD_IN_B], npix);
  if (!S.ok())
    return S.status();
  int rc = bs_building_map_dev(ctx, d_mask, width, height, d_map, out);
  if (rc != BS_OK)
    return rc;
  FreeUnlessKept<bs_buildings, bs_buildings_free> guard{out};
  S.download(map, d_map, npix);
  rc = S.finish();
  guard.keep = rc == BS_OK;
  return rc;
}

extern "C" int bs_assign_buildings_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, double ground_th,
                                       const int32_t* d_map, int32_t width, int32_t height, int32_t* d_building_idx,
                                       bs_buildings* inout)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_xyz || !d_map || !d_building_idx || !inout || n < 1 || bin < 1 || bad_raster(width, height) ||
      inout->n_buildings < 0 || inout->width != width || inout->height != height || !inout->n_points || !inout->n_above ||
      !inout->z_min || !inout->z_max || !inout->z_sum)
    return fail(ctx, BS_ERR_INVALID, "assign buildings: null pointer, n < 1, bin < 1 or a struct of another raster");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "assign buildings: 2^29 points or more");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int32_t nb = inout->n_buildings;
  const size_t m = (size_t)std::max(nb, 1);
  DevBuf* B = ctx->bd;
  Events<2> ev;
  for (int k = 0; k < 2; k++)
    BS_HIP(ctx, hipEventCreate(&ev.e[k]));
  BS_HIP(ctx, B[BD_FIG].reserve(32 * m));
  BS_HIP(ctx, B[BD_MISC].reserve(64));
  PtFig f;
  f.n_points = B[BD_FIG].as<unsigned long long>();
  f.n_above = f.n_points + m;
  f.z_sum = f.n_above + m;
  f.z_min = reinterpret_cast<int32_t*>(f.z_sum + m);
  f.z_max = f.z_min + m;
  int* d_bad = B[BD_MISC].as<int>();
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, st));
  if (nb > 0)
    ptfig_init_kernel<<<nblk(nb, 256), 256, 0, st>>>(f, nb);
  assign_kernel<<<(int)std::min<int64_t>(nblk(n, 256), 2048), 256, 0, st>>>(d_xyz, n, bin, ground_th, ground_rule(ctx), d_map, width, height,
                                                                          nb, d_building_idx, f, d_bad);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  int h_bad = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_bad)
    return fail(ctx, BS_ERR_RANGE, "assign buildings: a point's pixel lies outside the image (cloud not shifted, or another bin?)");
  if (nb > 0) {
    BS_HIP(ctx, hipMemcpyAsync(inout->n_points, f.n_points, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(inout->n_above, f.n_above, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(inout->z_sum, f.z_sum, 8 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(inout->z_min, f.z_min, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(inout->z_max, f.z_max, 4 * (size_t)nb, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
  }
  inout->ms_assign = ev.ms(0, 1);
  return BS_OK;
}

extern "C" int bs_assign_buildings(bs_ctx* ctx, const int32_t* xyz, int64_t n, int32_t bin, double ground_th,
                                   const int32_t* map, int32_t width, int32_t height, int32_t* building_idx,
                                   bs_buildings* inout)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!xyz || !map || !building_idx || !inout || n < 1 || bin < 1 || bad_raster(width, height))
    return fail(ctx, BS_ERR_INVALID, "assign buildings: null pointer, n < 1, bin < 1 or bad raster size");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "assign buildings: 2^29 points or more");
  DevBuf* B = ctx->bd;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(B[BD_IN_A], xyz, 3 * (size_t)n);
  const int32_t* d_map = S.upload(B[BD_IN_B], map, (size_t)width * height);
  int32_t* d_idx = S.room<int32_t>(B[BD_IN_C], (size_t)n);
  if (!S.ok())
    return S.status();
  const int rc = bs_assign_buildings_dev(ctx, d_xyz, n, bin, ground_th, d_map, width, height, d_idx, inout);
  if (rc != BS_OK)
    return rc;
  S.download(building_idx, d_idx, (size_t)n);
  return S.finish();
}

extern "C" int bs_plane_buildings_dev(bs_ctx* ctx, const int32_t* d_plane_idx, const int32_t* d_building_idx, int64_t n,
                                      int32_t n_planes, int32_t n_buildings, int32_t* plane_building, int64_t* votes_in,
                                      int64_t* votes_total, int64_t* votes_outside)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_plane_idx || !d_building_idx || n < 1 || n_planes < 0 || n_buildings < 0 ||
      (n_planes > 0 && (!plane_building || !votes_in || !votes_total || !votes_outside)))
    return fail(ctx, BS_ERR_INVALID, "plane buildings: null pointer, n < 1, n_planes < 0 or n_buildings < 0");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "plane buildings: 2^29 points or more");
  if (n_planes == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int32_t nb = n_buildings, npl = n_planes;
  const int64_t cells = (int64_t)npl * (nb + 1ll);
  DevBuf* B = ctx->bd;
  BS_HIP(ctx, B[BD_VOTE].reserve(24 * (size_t)npl));
  BS_HIP(ctx, B[BD_MISC].reserve(64));
  Votes v;
  v.total = B[BD_VOTE].as<unsigned long long>();
  v.outside = v.total + npl;
  v.best = v.outside + npl;
  int* d_bad = B[BD_MISC].as<int>();
  int32_t* d_nruns = d_bad + 1;
  BS_HIP(ctx, hipMemsetAsync(v.total, 0, 24 * (size_t)npl, st));
  BS_HIP(ctx, hipMemsetAsync(d_bad, 0, 8, st));
  const int grid = (int)std::min<int64_t>(nblk(n, 256), 2048);
  if (cells <= VOTE_DENSE_CELLS) {
    BS_HIP(ctx, B[BD_KEYS].reserve(4 * (size_t)cells));
    unsigned* hist = B[BD_KEYS].as<unsigned>();
    BS_HIP(ctx, hipMemsetAsync(hist, 0, 4 * (size_t)cells, st));
    if (cells <= VOTE_LDS_CELLS)
      vote_hist_kernel<true><<<grid, 256, 0, st>>>(d_plane_idx, d_building_idx, n, npl, nb, (int32_t)cells, hist, d_bad);
    else
      vote_hist_kernel<false><<<grid, 256, 0, st>>>(d_plane_idx, d_building_idx, n, npl, nb, (int32_t)cells, hist, d_bad);
    vote_cells_kernel<<<nblk(cells, 256), 256, 0, st>>>(hist, cells, nb, v);
  } else {
    const uint64_t none = (uint64_t)cells;  // sorts behind every cell
    int bits = 1;
    while ((1ull << bits) <= none)
      bits++;
    BS_HIP(ctx, B[BD_KEYS].reserve(8 * (size_t)n));
    BS_HIP(ctx, B[BD_KEYS2].reserve(8 * (size_t)n));
    BS_HIP(ctx, B[BD_RUNS].reserve(12 * (size_t)n));
    uint64_t* keys = B[BD_KEYS].as<uint64_t>();
    uint64_t* sorted = B[BD_KEYS2].as<uint64_t>();
    uint64_t* run_key = B[BD_RUNS].as<uint64_t>();
    int32_t* run_len = reinterpret_cast<int32_t*>(run_key + n);
    vote_keys_kernel<<<nblk(n, 256), 256, 0, st>>>(d_plane_idx, d_building_idx, n, npl, nb, none, keys, d_bad);
    auto sort = [&](void* tmp, size_t& bytes) { return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys, sorted, (int)n, 0, bits, st); };
    auto runs = [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceRunLengthEncode::Encode(tmp, bytes, sorted, run_key, run_len, d_nruns, (int)n, st);
    };
    BS_HIP(ctx, cub_room(B[BD_TMP], sort, runs));
    BS_HIP(ctx, cub_run(B[BD_TMP], sort));
    BS_HIP(ctx, cub_run(B[BD_TMP], runs));
    vote_runs_kernel<<<nblk(n, 256), 256, 0, st>>>(run_key, run_len, d_nruns, none, nb, v);
  }
  std::vector<unsigned long long> hv(3 * (size_t)npl);
  int h_bad = 0;
  BS_HIP(ctx, hipMemcpyAsync(hv.data(), v.total, 24 * (size_t)npl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_bad)
    return fail(ctx, BS_ERR_RANGE, "plane buildings: a building index outside [-1, n_buildings)");
  for (int32_t p = 0; p < npl; p++) {
    const unsigned long long best = hv[2 * (size_t)npl + p];
    votes_total[p] = (int64_t)hv[p];
    votes_outside[p] = (int64_t)hv[(size_t)npl + p];
    votes_in[p] = (int64_t)(best >> 32);
    plane_building[p] = best ? (int32_t)(0xFFFFFFFFu - (uint32_t)best) : -1;
  }
  return BS_OK;
}

extern "C" int bs_plane_buildings(bs_ctx* ctx, const int32_t* plane_idx, const int32_t* building_idx, int64_t n,
                                  int32_t n_planes, int32_t n_buildings, int32_t* plane_building, int64_t* votes_in,
                                  int64_t* votes_total, int64_t* votes_outside)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!plane_idx || !building_idx || n < 1 || n_planes < 0 || n_buildings < 0)
    return fail(ctx, BS_ERR_INVALID, "plane buildings: null pointer, n < 1, n_planes < 0 or n_buildings < 0");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "plane buildings: 2^29 points or more");
  Staging S(ctx);
  const int32_t* d_plane = S.upload(ctx->bd[BD_IN_A], plane_idx, (size_t)n);
  const int32_t* d_building = S.upload(ctx->bd[BD_IN_C], building_idx, (size_t)n);
  if (!S.ok())
    return S.status();
  // (the results are host arrays that the device form fills and waits for: nothing to download or finish)
  return bs_plane_buildings_dev(ctx, d_plane, d_building, n, n_planes, n_buildings, plane_building, votes_in, votes_total,
                                votes_outside);
}

// The format is written down in include/bs_api.h.
extern "C" int bs_buildings_write_obj(const bs_contours* c, const bs_buildings* b, int32_t bin, const int32_t* origin,
                                      double ground_th, double min_area, double min_perimeter, const char* path)
{
  if (!c || !b || !path || bin < 1 || c->n_contours < 0 || c->n_contours != b->n_buildings ||
      (c->n_contours > 0 && (!c->offset || !c->xy || !c->area || !c->perimeter || !b->n_above || !b->z_sum)))
    return BS_ERR_INVALID;
  FILE* f = fopen(path, "w");
  if (!f)
    return BS_ERR_INVALID;
  const int64_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  std::vector<int32_t> kept;
  for (int32_t i = 0; i < c->n_contours; i++)
    if (c->area[i] > min_area && c->perimeter[i] > min_perimeter && b->n_above[i] > 0)
      kept.push_back(i);
  fprintf(f, "# buildings: %d of %d\n", (int)kept.size(), c->n_contours);
  const long long z0 = (long long)((int64_t)ground_th + o[2]);
  for (int32_t i : kept) {
    const long long z1 = (long long)(b->z_sum[i] / b->n_above[i] + o[2]);
    for (int64_t k = c->offset[i]; k < c->offset[i + 1]; k++) {
      const long long x = (long long)c->xy[2 * k] * bin + o[0], y = (long long)c->xy[2 * k + 1] * bin + o[1];
      fprintf(f, "v %lld %lld %lld\nv %lld %lld %lld\n", x, y, z0, x, y, z1);
    }
  }
  int64_t base = 1;
  for (int32_t i : kept) {  // my_function.cpp:109-126
    const int64_t n = c->offset[i + 1] - c->offset[i];
    for (int64_t k = 0; k < n; k++) {
      const int64_t nx = (k + 1) % n;
      fprintf(f, "f %lld %lld %lld %lld\n", (long long)(base + 2 * k), (long long)(base + 2 * nx),
              (long long)(base + 2 * nx + 1), (long long)(base + 2 * k + 1));
    }
    base += 2 * n;
  }
  base = 1;
  for (int32_t i : kept) {  // the roof: the top vertices in contour order
    const int64_t n = c->offset[i + 1] - c->offset[i];
    if (n >= 3) {
      fputc('f', f);
      for (int64_t k = 0; k < n; k++)
        fprintf(f, " %lld", (long long)(base + 2 * k + 1));
      fputc('\n', f);
    }
    base += 2 * n;
  }
  const bool ok = !ferror(f);
  return (fclose(f) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}
