// bs_contour.hip -- building footprints: the reference's extracted_contour (/root/reference/tmc3/my_function.cpp:8-145)
// on the density raster of bs_grid_picture, without OpenCV and without leaving the device until the point lists are
// complete.  Stages ("Building footprints"):
//   1. mask   f64 max of channel 1 (integer atomicMax on the bits of non-negative doubles), then one pass that
//             quantises like save_image, thresholds, and writes a (W+2) x (H+2) byte mask with a zero frame
//             (findContours' one-pixel padding)
//   2. close  `iterations` dilations then as many erosions, one LDS-tiled pass each; the ellipse is a union of
//             centred horizontal runs, so a pass is an OR / AND over the rows dy of a run of half-width dx(dy)
//   3. label  union-find over the padded grid (bs_uf.h, parent <= self): foreground 8-connected, background
//             4-connected; a root is its component's first raster pixel, i.e. findContours' start pixel i0.  A
//             component is external iff the background pixel above i0 has the frame's root.
//   4. trace  every (pixel, back-direction) state of the border pixels of external components gets its successor
//             under OpenCV's follower; the state that leads into a start state (i0, s_init) is a list tail, so each
//             outer border becomes a list, ranked by Wyllie pointer jumping with weights = "emits a point"
//             (CHAIN_APPROX_SIMPLE: s != b ^ 4).  Hole borders stay cycles and are never read.
//   5. output contours in descending i0, emitted points scattered by rank, area / perimeter in exact arithmetic.
// There is one code path: footprints_tiles_dev works on a batch of tiles (DESIGN.md §4 "Batches of rasters and
// footprints"), and the solo call bs_footprints_dev is that batch with one tile.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bs_common.h"
#include "bs_host.h"
#include "bs_uf.h"

namespace bs {
namespace {

// the staging slots of the host forms in bs_ctx::fp (0 .. 20: the scratch of footprints_tiles_dev, by number there)
enum { FP_IN_IMAGE = 21, FP_OUT_MASK, FP_COUNT };
static_assert(FP_COUNT <= (int)(sizeof(bs_ctx::fp) / sizeof(DevBuf)), "bs_ctx::fp is too short");

constexpr int32_t END = -1;
constexpr int TW = 64, TH = 16, RMAX = 7;  // closing tile (outputs) and the largest ellipse radius (15 x 15)
enum : uint8_t { K_INVALID = 0, K_NORMAL = 1, K_TAIL = 2, K_DEAD = 3, K_EMIT = 4 };

struct Ellipse {
  int r;
  int dx[2 * RMAX + 1];  // half-width of the centred run of row dy = i - r
};

// OpenCV's chain codes in (x, y), y down: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE
__device__ inline int delta(int s, int wp)
{
  const int dx = (s == 0 || s == 1 || s == 7) ? 1 : (s >= 3 && s <= 5) ? -1 : 0;
  const int dy = (s >= 1 && s <= 3) ? -1 : (s >= 5) ? 1 : 0;
  return dy * wp + dx;
}

// findContours' first search around an outer start pixel: s = 3, 2, 1, 0, 7, 6, 5 (clockwise from W); -1: none
__device__ inline int first_search(const uint8_t* m, int p, int wp)
{
  for (int s = 3; s != 4; s = (s - 1) & 7)
    if (m[p + delta(s, wp)])
      return s;
  return -1;
}

// The padded masks of a batch lie one after another: tile t's (W+2) x (H+2) array starts at pbase, its image at pixel
// ibase of the batch image and its closing blocks at bbase.  Isolation invariant: no union, neighbour read or successor
// step leaves its tile's padded array.  Every row / column test is made on the TILE-LOCAL index i - pbase with the
// tile's own wp; since every tile has its own zero frame, a foreground pixel's 8 neighbours and a (y > 0, x > 0)
// pixel's W, N, NW, NE neighbours all lie in the same array.  (Tested on the global index, the first frame row of a
// wide tile would look N into the middle of the narrower tile before it.)  Labels, flags, scans and list ranking then
// work on global indices; a tile's frame root is pbase.  A solo call is the batch of one tile: all bases are 0.
struct FpTile {
  int32_t w, h, wp;
  int32_t pbase;  // first padded pixel
  int32_t ibase;  // first image pixel
  int32_t bbase;  // first closing block
  int32_t bx;     // closing blocks per row
  int32_t pad_;
};

struct PixBlock {  // up to MAX_CHUNK image pixels of ONE tile (segmented max)
  int32_t tile, begin, end;
};
constexpr int MAX_CHUNK = 4096;

// mx[t] = the bits of max(0, max channel 1 of tile t); a block takes up to MAX_CHUNK pixels of one tile
__global__ __launch_bounds__(256) void max_tiled_kernel(const double* __restrict__ img, const PixBlock* __restrict__ blk,
                                                        unsigned long long* __restrict__ mx)
{
  const PixBlock b = blk[blockIdx.x];
  double m = 0;  // the reference's loop starts at 0; NaN never wins a comparison
  for (int64_t i = b.begin + (int64_t)threadIdx.x; i < b.end; i += blockDim.x) {
    const double v = img[3 * i + 1];
    if (v > m)
      m = v;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(m, o);
    if (t > m)
      m = t;
  }
  __shared__ double w[4];
  if ((threadIdx.x & 63) == 0)
    w[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; k++)
      if (w[k] > m)
        m = w[k];
    if (m > 0)  // non-negative doubles order like their bit patterns
      atomicMax(mx + b.tile, (unsigned long long)__double_as_longlong(m));
  }
}

__global__ __launch_bounds__(256) void mask_tiled_kernel(const double* __restrict__ img, const FpTile* __restrict__ tiles,
                                                         const int32_t* __restrict__ pb, int32_t nt, int64_t np, int thr,
                                                         const unsigned long long* __restrict__ mx,
                                                         const uint8_t* __restrict__ screen, uint8_t* __restrict__ m)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= np)
    return;
  const int32_t t = tile_of(pb, nt, i);
  const FpTile T = tiles[t];
  const int32_t li = (int32_t)i - T.pbase;
  const int32_t y = li / T.wp, x = li - y * T.wp;
  uint8_t v = 0;
  if (x >= 1 && x <= T.w && y >= 1 && y <= T.h) {
    const double max1 = __longlong_as_double((long long)mx[t]);
    if (max1 != 0) {  // save_image, TMC3.cpp:100-108: (uint8)(255.0 * (1.0 * v / max1))
      const double q0 = 255.0 * (1.0 * img[3 * ((int64_t)T.ibase + (int64_t)(y - 1) * T.w + (x - 1)) + 1] / max1);
      const int q = q0 > 0 ? (int)q0 : 0;
      v = q > thr;  // threshold(..., 10, 255, THRESH_BINARY), my_function.cpp:20
      if (screen)  // bs_set_footprint_screen: one tile, whose image is the screen's
        v &= screen[(int64_t)(y - 1) * T.w + (x - 1)] != 0;
    }
  }
  m[i] = v;
}

// one dilation (OR) or erosion (AND) of the interiors; outside its image counts as 0 (dilate) / 1 (erode).  The block
// grid is flattened: block -> (tile, block column, block row)
template <bool DILATE>
__global__ __launch_bounds__(256) void morph_tiled_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                          const FpTile* __restrict__ tiles, const int32_t* __restrict__ bb,
                                                          int32_t nt, Ellipse e)
{
  __shared__ uint8_t t[(TH + 2 * RMAX) * (TW + 2 * RMAX)];
  const FpTile T = tiles[tile_of(bb, nt, blockIdx.x)];
  const int lb = (int)blockIdx.x - T.bbase, by = lb / T.bx;
  const int r = e.r, lw = TW + 2 * r, lh = TH + 2 * r;
  const int x0 = (lb - by * T.bx) * TW, y0 = by * TH;
  const int w = T.w, h = T.h;
  const int64_t wp = T.wp;
  src += T.pbase;
  dst += T.pbase;
  for (int k = threadIdx.x; k < lw * lh; k += blockDim.x) {
    const int ly = k / lw, lx = k - ly * lw;
    const int gx = x0 + lx - r, gy = y0 + ly - r;
    uint8_t v = DILATE ? 0 : 1;
    if (gx >= 0 && gx < w && gy >= 0 && gy < h)
      v = src[(gy + 1) * wp + gx + 1];
    t[k] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x & 63, ty0 = (threadIdx.x >> 6) * 4;
  const int gx = x0 + tx;
  if (gx >= w)
    return;
  for (int j = 0; j < 4; j++) {
    const int ty = ty0 + j, gy = y0 + ty;
    if (gy >= h)
      break;
    uint8_t acc = DILATE ? 0 : 1;
    for (int dy = -r; dy <= r; dy++) {
      const int d = e.dx[dy + r];
      const uint8_t* row = t + (ty + r + dy) * lw + tx + r;
      for (int dx = -d; dx <= d; dx++) {
        if (DILATE)
          acc |= row[dx];
        else
          acc &= row[dx];
      }
    }
    dst[(gy + 1) * wp + gx + 1] = acc;
  }
}

__global__ __launch_bounds__(256) void cc_init_kernel(int32_t* __restrict__ parent, int64_t np)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < np)
    parent[i] = (int32_t)i;
}

// foreground joins its W, N, NW, NE neighbours (8-connectivity), background its W and N ones (4-connectivity); the row /
// column tests are tile-local (the isolation invariant above)
__global__ __launch_bounds__(256) void cc_union_tiled_kernel(const uint8_t* __restrict__ m, const FpTile* __restrict__ tiles,
                                                             const int32_t* __restrict__ pb, int32_t nt, int64_t np,
                                                             int32_t* parent)
{
  const int64_t i64 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i64 >= np)
    return;
  const int32_t i = (int32_t)i64;
  const FpTile T = tiles[tile_of(pb, nt, i)];
  const int32_t wp = T.wp, li = i - T.pbase;
  const int32_t y = li / wp, x = li - y * wp;
  const uint8_t v = m[i];
  const bool w_same = x > 0 && m[i - 1] == v;
  if (w_same)
    uf_union(parent, i, i - 1);
  if (y > 0) {
    // N is already joined to W through NW when all three share the class
    if (m[i - wp] == v && !(w_same && m[i - wp - 1] == v))
      uf_union(parent, i, i - wp);
    if (v) {
      if (x > 0 && m[i - wp - 1] && !m[i - wp] && !w_same)
        uf_union(parent, i, i - wp - 1);
      if (x < wp - 1 && m[i - wp + 1] && !m[i - wp])
        uf_union(parent, i, i - wp + 1);
    }
  }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* parent, int64_t np)
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

// bflag: foreground pixel of an external component with a background 8-neighbour (a tracer state owner);
// rflag: start pixel i0 of an external component.  External iff the pixel above the root has the tile's frame root pbase
__global__ __launch_bounds__(256) void flags_tiled_kernel(const uint8_t* __restrict__ m, const int32_t* __restrict__ parent,
                                                          const FpTile* __restrict__ tiles, const int32_t* __restrict__ pb,
                                                          int32_t nt, int64_t np, int32_t* __restrict__ bflag,
                                                          int32_t* __restrict__ rflag,
                                                          unsigned long long* __restrict__ n_fg)
{
  const int64_t i64 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int32_t i = (int32_t)i64;
  const bool fg = i64 < np && m[i];
  int32_t b = 0, r = 0;
  if (fg) {  // foreground never lies on the frame: all 8 neighbours exist
    const FpTile T = tiles[tile_of(pb, nt, i)];
    const int32_t root = parent[i];
    if (parent[root - T.wp] == T.pbase) {
      r = root == i;
      for (int s = 0; s < 8; s++)
        b |= !m[i + delta(s, T.wp)];
    }
  }
  const unsigned long long bal = __ballot(fg);
  if ((threadIdx.x & 63) == 0 && bal)
    atomicAdd(n_fg, (unsigned long long)__popcll(bal));
  if (i64 >= np)
    return;
  bflag[i] = b;
  rflag[i] = r;
}

// rb[t] = external components before tile t (t = 0 .. nt): tile t's contours are [rb[t], rb[t+1])
__global__ void rbase_kernel(const int32_t* __restrict__ rflag, const int32_t* __restrict__ rscan,
                             const int32_t* __restrict__ pb, int32_t nt, int64_t np, int32_t* __restrict__ rb)
{
  const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > nt)
    return;
  rb[t] = t < nt ? rscan[pb[t]] : rscan[np - 1] + rflag[np - 1];
}

// contours by (tile ascending, i0 descending): the r-th start pixel of the batch, in tile t, is contour
// rb[t] + rb[t+1] - 1 - r
__device__ inline int32_t contour_of(const int32_t* rb, int32_t t, int32_t r) { return rb[t] + rb[t + 1] - 1 - r; }

__global__ __launch_bounds__(256) void lists_kernel(const int32_t* __restrict__ bflag, const int32_t* __restrict__ bscan,
                                                    const int32_t* __restrict__ rflag, const int32_t* __restrict__ rscan,
                                                    int64_t np, int32_t* __restrict__ bpix, int32_t* __restrict__ rpix)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= np)
    return;
  if (bflag[i])
    bpix[bscan[i]] = (int32_t)i;
  if (rflag[i])
    rpix[rscan[i]] = (int32_t)i;
}

// state st = 8 * (border pixel id) + b, b = code pointing back at the previous contour pixel
__global__ __launch_bounds__(256) void state_tiled_kernel(const uint8_t* __restrict__ m, const FpTile* __restrict__ tiles,
                                                          const int32_t* __restrict__ pb, int32_t nt,
                                                          const int32_t* __restrict__ bpix,
                                                          const int32_t* __restrict__ bflag,
                                                          const int32_t* __restrict__ bscan,
                                                          const int32_t* __restrict__ rflag, int64_t ns,
                                                          int32_t* __restrict__ succ, uint8_t* __restrict__ kind,
                                                          int32_t* __restrict__ nxt, uint32_t* __restrict__ val,
                                                          int32_t* __restrict__ last)
{
  const int64_t st64 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (st64 >= ns)
    return;
  const int32_t st = (int32_t)st64;
  const int b = st & 7;
  const int32_t p = bpix[st >> 3];
  const int wp = tiles[tile_of(pb, nt, p)].wp;
  int32_t sc = END, nx = END;
  uint32_t w = 0;
  uint8_t k = K_INVALID;
  if (m[p + delta(b, wp)]) {
    int s = b;
    do {  // the follower: counter-clockwise from b + 1; stops at b at the latest
      s = (s + 1) & 7;
    } while (!m[p + delta(s, wp)]);
    w = s != (b ^ 4);  // CHAIN_APPROX_SIMPLE keeps the pixel iff the direction changes
    const int32_t q = p + delta(s, wp);
    const int b2 = (s + 4) & 7;
    if (!bflag[q]) {
      k = K_DEAD;
    } else {
      sc = bscan[q] * 8 + b2;
      if (rflag[q] && first_search(m, q, wp) == b2) {
        k = K_TAIL;  // leads into a start state: cut the cycle here
      } else {
        k = K_NORMAL;
        nx = sc;
      }
    }
  }
  succ[st] = sc;
  kind[st] = k | (w ? K_EMIT : 0);
  nxt[st] = nx;
  val[st] = w;
  last[st] = st;
}

// one Wyllie round: segment [st, nxt) absorbs [nxt, nxt[nxt]); val = emitted states in the segment, last = its last
__global__ __launch_bounds__(256) void jump_kernel(const int32_t* __restrict__ nxt, const uint32_t* __restrict__ val,
                                                   const int32_t* __restrict__ last, int64_t ns,
                                                   int32_t* __restrict__ nxt2, uint32_t* __restrict__ val2,
                                                   int32_t* __restrict__ last2)
{
  const int64_t st = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (st >= ns)
    return;
  const int32_t j = nxt[st];
  if (j == END) {
    nxt2[st] = END;
    val2[st] = val[st];
    last2[st] = last[st];
  } else {
    nxt2[st] = nxt[j];
    val2[st] = val[st] + val[j];  // (cycles wrap; their values are never read)
    last2[st] = last[j];
  }
}

// the emitted count and the start state of the contour of every start pixel
__global__ __launch_bounds__(256) void contour_count_tiled_kernel(const uint8_t* __restrict__ m,
                                                                  const FpTile* __restrict__ tiles,
                                                                  const int32_t* __restrict__ pb, int32_t nt,
                                                                  const int32_t* __restrict__ rb,
                                                                  const int32_t* __restrict__ rpix, int32_t nc,
                                                                  const int32_t* __restrict__ bscan,
                                                                  const int32_t* __restrict__ succ,
                                                                  const uint8_t* __restrict__ kind,
                                                                  const int32_t* __restrict__ nxt,
                                                                  const uint32_t* __restrict__ val,
                                                                  const int32_t* __restrict__ last,
                                                                  int64_t* __restrict__ cnt,
                                                                  int32_t* __restrict__ cstart, int* __restrict__ err)
{
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nc)
    return;
  const int32_t i = rpix[r], t = tile_of(pb, nt, i), c = contour_of(rb, t, r);
  const int s0 = first_search(m, i, tiles[t].wp);
  if (s0 < 0) {  // a single pixel: [i0]
    cnt[c] = 1;
    cstart[c] = -1;
    return;
  }
  const int32_t st = bscan[i] * 8 + s0;
  const int32_t tl = last[st];
  if (nxt[st] != END || (kind[tl] & 3) != K_TAIL || succ[tl] != st) {
    atomicOr(err, 1);  // the list did not close within the round bound
    cnt[c] = 0;
    cstart[c] = -2;
    return;
  }
  cnt[c] = val[st];
  cstart[c] = st;
}

__global__ __launch_bounds__(256) void scatter_tiled_kernel(const FpTile* __restrict__ tiles, const int32_t* __restrict__ pb,
                                                            int32_t nt, const int32_t* __restrict__ rb,
                                                            const int32_t* __restrict__ bpix,
                                                            const int32_t* __restrict__ rscan,
                                                            const int32_t* __restrict__ succ,
                                                            const uint8_t* __restrict__ kind,
                                                            const int32_t* __restrict__ nxt,
                                                            const uint32_t* __restrict__ val,
                                                            const int32_t* __restrict__ last, int64_t ns,
                                                            const int64_t* __restrict__ off, int32_t* __restrict__ xy,
                                                            int32_t* __restrict__ cid, int* __restrict__ err)
{
  const int64_t st = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (st >= ns)
    return;
  const uint8_t k = kind[st];
  if (!(k & K_EMIT) || (k & 3) == K_DEAD || nxt[st] != END)
    return;
  const int32_t tl = last[st];
  if ((kind[tl] & 3) != K_TAIL)
    return;  // a dead chain
  const int32_t start = succ[tl];
  const int32_t s0 = bpix[start >> 3], t = tile_of(pb, nt, s0);  // (a list never leaves its tile: st's tile too)
  const int32_t c = contour_of(rb, t, rscan[s0]);
  const int64_t pos = off[c] + (int64_t)(val[start] - val[st]);
  if (pos < off[c] || pos >= off[c + 1]) {
    atomicOr(err, 2);
    return;
  }
  const FpTile T = tiles[t];
  const int32_t li = bpix[st >> 3] - T.pbase, y = li / T.wp, x = li - y * T.wp;
  xy[2 * pos] = x - 1;
  xy[2 * pos + 1] = y - 1;
  cid[pos] = c;
}

__global__ __launch_bounds__(256) void single_tiled_kernel(const FpTile* __restrict__ tiles, const int32_t* __restrict__ pb,
                                                           int32_t nt, const int32_t* __restrict__ rb,
                                                           const int32_t* __restrict__ rpix,
                                                           const int32_t* __restrict__ cstart, int32_t nc,
                                                           const int64_t* __restrict__ off, int32_t* __restrict__ xy,
                                                           int32_t* __restrict__ cid)
{
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nc)
    return;
  const int32_t p = rpix[r], t = tile_of(pb, nt, p), c = contour_of(rb, t, r);
  if (cstart[c] != -1)
    return;
  const FpTile T = tiles[t];
  const int32_t li = p - T.pbase, y = li / T.wp, x = li - y * T.wp;
  xy[2 * off[c]] = x - 1;
  xy[2 * off[c] + 1] = y - 1;
  cid[off[c]] = c;
}

// per point: the shoelace term (exact in int64) and the float segment length from the previous point as an integer
// multiple of 2^-23 (every non-zero length is >= 1, hence such a multiple); wave-aggregated atomics per contour
__global__ __launch_bounds__(256) void measure_kernel(const int32_t* __restrict__ xy, const int32_t* __restrict__ cid,
                                                      const int64_t* __restrict__ off, int64_t total, int32_t nc,
                                                      unsigned long long* __restrict__ asum,
                                                      unsigned long long* __restrict__ psum)
{
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  int32_t c = -1;
  unsigned long long a = 0, l = 0;
  if (k < total)
    c = cid[k];
  if (c >= nc)
    c = -1;  // (every position is written exactly once; this only keeps a broken invariant in bounds)
  if (c >= 0) {
    const int64_t pk = k == off[c] ? off[c + 1] - 1 : k - 1;
    const int32_t x = xy[2 * k], y = xy[2 * k + 1], px = xy[2 * pk], py = xy[2 * pk + 1];
    a = (unsigned long long)((int64_t)px * y - (int64_t)py * x);
    const float dx = (float)x - (float)px, dy = (float)y - (float)py;
    const float len = sqrtf(dx * dx + dy * dy);
    l = (unsigned long long)((double)len * 8388608.0);
  }
  const int32_t c0 = __shfl(c, 0);
  if (__all(c == c0) && c0 >= 0) {
    for (int o = 32; o > 0; o >>= 1) {
      a += __shfl_xor(a, o);
      l += __shfl_xor(l, o);
    }
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(asum + c0, a);
      atomicAdd(psum + c0, l);
    }
  } else if (c >= 0) {
    atomicAdd(asum + c, a);
    atomicAdd(psum + c, l);
  }
}

// contourArea = |sum| * 0.5; arcLength: the reference sums float lengths into a double in point order, which is
// exact (and so equal to the integer sum) while the total stays below 2^30; otherwise sum sequentially here
__global__ __launch_bounds__(256) void finish_kernel(const int32_t* __restrict__ xy, const int64_t* __restrict__ off,
                                                     int32_t nc, const unsigned long long* __restrict__ asum,
                                                     const unsigned long long* __restrict__ psum,
                                                     double* __restrict__ area, double* __restrict__ perim)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc)
    return;
  const int64_t s = (int64_t)asum[c];
  area[c] = fabs((double)s * 0.5);
  if (psum[c] < (1ull << 53)) {
    perim[c] = (double)psum[c] / 8388608.0;
    return;
  }
  const int64_t a = off[c], e = off[c + 1];
  double per = 0;
  float px = (float)xy[2 * (e - 1)], py = (float)xy[2 * (e - 1) + 1];
  for (int64_t k = a; k < e; k++) {
    const float x = (float)xy[2 * k], y = (float)xy[2 * k + 1];
    const float dx = x - px, dy = y - py;
    per += sqrtf(dx * dx + dy * dy);
    px = x;
    py = y;
  }
  perim[c] = per;
}

__global__ __launch_bounds__(256) void mask_out_tiled_kernel(const uint8_t* __restrict__ m, const FpTile* __restrict__ tiles,
                                                             const int32_t* __restrict__ ib, int32_t nt, int64_t npix,
                                                             uint8_t* __restrict__ out)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= npix)
    return;
  const FpTile T = tiles[tile_of(ib, nt, i)];
  const int32_t li = (int32_t)i - T.ibase, y = li / T.w, x = li - y * T.w;
  out[i] = m[T.pbase + (int64_t)(y + 1) * T.wp + x + 1] ? 255 : 0;
}

// getStructuringElement(MORPH_ELLIPSE, Size(s, s)): row i has the run c - dx .. c + dx,
// dx = cvRound(c * sqrt((r*r - dy*dy) / (r*r))), dy = i - r, r = c = s / 2
Ellipse make_ellipse(int s)
{
  Ellipse e{};
  e.r = s / 2;
  const int r = e.r, c = s / 2;
  const double inv_r2 = r ? 1.0 / ((double)r * r) : 0;
  for (int i = 0; i < s; i++) {
    const int dy = i - r;
    const int dx = (int)std::nearbyint(c * std::sqrt((r * r - dy * dy) * inv_r2));  // round half to even
    e.dx[i] = std::min(dx, c);
  }
  return e;
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_contours_free(bs_contours* c)
{
  if (!c)
    return;
  free(c->offset);
  free(c->xy);
  free(c->area);
  free(c->perimeter);
  memset(c, 0, sizeof *c);
}

namespace {

using ContoursGuard = FreeUnlessKept<bs_contours, bs_contours_free>;

// fail() with the caller's name in front: "footprints" for the solo call, "footprints batch" for a batch
int fail_as(bs_ctx* ctx, int status, const char* who, const char* what)
{
  char msg[160];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return fail(ctx, status, msg);
}

// The footprints of n_tiles rasters in one pass.  The callers have checked every argument: the sizes are positive and
// the padded pixels of all tiles together stay below 2^31.  out->width / height stay 0.
int footprints_tiles_dev(bs_ctx* ctx, const double* d_image, const int32_t* width, const int32_t* height,
                         int32_t n_tiles, int32_t threshold, int32_t kernel_size, int32_t iterations, uint8_t* d_mask,
                         bs_contours* out, int32_t* contour_offset, bs_footprint_info* info, const char* who)
{
  const int32_t nt = n_tiles;
  if (ctx->fs_ptr && nt > 1)
    return fail(ctx, BS_ERR_INVALID, "footprints batch: more than one tile while a footprint screen is set (bs_set_footprint_screen)");
  if (ctx->fs_ptr && (width[0] != ctx->fs_w || height[0] != ctx->fs_h))
    return fail(ctx, BS_ERR_INVALID, "footprints: the raster's width / height differ from the footprint screen's");
  std::vector<FpTile> tl(nt);
  std::vector<int32_t> pb(nt + 1), ib(nt + 1), bb(nt + 1);
  std::vector<PixBlock> blk;
  int64_t np = 0, npix = 0, nblocks = 0;
  for (int32_t t = 0; t < nt; t++) {
    const int32_t w = width[t], h = height[t];
    FpTile& T = tl[t];
    T.w = w;
    T.h = h;
    T.wp = w + 2;
    T.pbase = pb[t] = (int32_t)np;
    T.ibase = ib[t] = (int32_t)npix;
    T.bbase = bb[t] = (int32_t)nblocks;
    T.bx = nblk(w, TW);
    for (int64_t b = npix; b < npix + (int64_t)w * h; b += MAX_CHUNK)
      blk.push_back({t, (int32_t)b, (int32_t)std::min<int64_t>(npix + (int64_t)w * h, b + MAX_CHUNK)});
    np += (int64_t)(w + 2) * (h + 2);
    npix += (int64_t)w * h;
    nblocks += (int64_t)T.bx * nblk(h, TH);
  }
  pb[nt] = (int32_t)np;
  ib[nt] = (int32_t)npix;
  bb[nt] = (int32_t)nblocks;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // descriptors: FpTile [nt] | pb [nt+1] | ib [nt+1] | bb [nt+1] | PixBlock [blocks]
  const size_t s_t = sizeof(FpTile) * nt, s_o = sizeof(int32_t) * (nt + 1);
  std::vector<char> desc(s_t + 3 * s_o + sizeof(PixBlock) * blk.size());
  memcpy(desc.data(), tl.data(), s_t);
  memcpy(desc.data() + s_t, pb.data(), s_o);
  memcpy(desc.data() + s_t + s_o, ib.data(), s_o);
  memcpy(desc.data() + s_t + 2 * s_o, bb.data(), s_o);
  memcpy(desc.data() + s_t + 3 * s_o, blk.data(), sizeof(PixBlock) * blk.size());
  BS_HIP(ctx, ctx->tile_desc.reserve(desc.size()));
  char* dd = ctx->tile_desc.as<char>();
  const FpTile* d_tl = reinterpret_cast<const FpTile*>(dd);
  const int32_t* d_pb = reinterpret_cast<const int32_t*>(dd + s_t);
  const int32_t* d_ib = reinterpret_cast<const int32_t*>(dd + s_t + s_o);
  const int32_t* d_bb = reinterpret_cast<const int32_t*>(dd + s_t + 2 * s_o);
  const PixBlock* d_blk = reinterpret_cast<const PixBlock*>(dd + s_t + 3 * s_o);
  BS_HIP(ctx, hipMemcpyAsync(dd, desc.data(), desc.size(), hipMemcpyHostToDevice, st));

  DevBuf* B = ctx->fp;
  Events<6> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));
  BS_HIP(ctx, B[0].reserve(np));
  BS_HIP(ctx, B[1].reserve(np));
  BS_HIP(ctx, B[2].reserve(4 * np));
  BS_HIP(ctx, B[3].reserve(4 * np));
  BS_HIP(ctx, B[4].reserve(4 * np));
  BS_HIP(ctx, B[5].reserve(4 * np));
  BS_HIP(ctx, B[6].reserve(4 * np));
  // misc: error flags | foreground count | per-tile max bits [nt] | contour bases rb [nt + 1]
  const size_t misc = 16 + 8 * (size_t)nt + 4 * (size_t)(nt + 1);
  BS_HIP(ctx, B[7].reserve(misc));
  uint8_t* mA = B[0].as<uint8_t>();
  uint8_t* mB = B[1].as<uint8_t>();
  int32_t* parent = B[2].as<int32_t>();
  int32_t* bflag = B[3].as<int32_t>();
  int32_t* bscan = B[4].as<int32_t>();
  int32_t* rflag = B[5].as<int32_t>();
  int32_t* rscan = B[6].as<int32_t>();
  int* d_err = B[7].as<int>();
  unsigned long long* d_fg = B[7].as<unsigned long long>() + 1;
  unsigned long long* d_mx = d_fg + 1;
  int32_t* d_rb = reinterpret_cast<int32_t*>(d_mx + nt);

  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(B[7].p, 0, misc, st));
  if (!blk.empty())
    max_tiled_kernel<<<(int)blk.size(), 256, 0, st>>>(d_image, d_blk, d_mx);
  mask_tiled_kernel<<<nblk(np, 256), 256, 0, st>>>(d_image, d_tl, d_pb, nt, np, threshold, d_mx, ctx->fs_ptr, mA);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));

  uint8_t* m = mA;
  if (iterations > 0) {
    const Ellipse e = make_ellipse(kernel_size);
    BS_HIP(ctx, hipMemsetAsync(mB, 0, np, st));  // the frames of the second buffer
    uint8_t* src = mA;
    uint8_t* dst = mB;
    for (int it = 0; it < 2 * iterations; it++) {
      if (it < iterations)
        morph_tiled_kernel<true><<<(unsigned)nblocks, 256, 0, st>>>(src, dst, d_tl, d_bb, nt, e);
      else
        morph_tiled_kernel<false><<<(unsigned)nblocks, 256, 0, st>>>(src, dst, d_tl, d_bb, nt, e);
      std::swap(src, dst);
    }
    m = src;
  }
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));

  cc_init_kernel<<<nblk(np, 256), 256, 0, st>>>(parent, np);
  cc_union_tiled_kernel<<<nblk(np, 256), 256, 0, st>>>(m, d_tl, d_pb, nt, np, parent);
  cc_flatten_kernel<<<nblk(np, 256), 256, 0, st>>>(parent, np);
  flags_tiled_kernel<<<nblk(np, 256), 256, 0, st>>>(m, parent, d_tl, d_pb, nt, np, bflag, rflag, d_fg);
  auto scan = [&](auto* count, auto* sum, int64_t n) {
    return [=](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, count, sum, (int)n, st); };
  };
  BS_HIP(ctx, cub_run(B[8], scan(bflag, bscan, np)));
  BS_HIP(ctx, cub_run(B[8], scan(rflag, rscan, np)));
  rbase_kernel<<<nblk(nt + 1, 256), 256, 0, st>>>(rflag, rscan, d_pb, nt, np, d_rb);
  std::vector<int32_t> h_rb(nt + 1);
  int32_t h_tail[2] = {0, 0};
  BS_HIP(ctx, hipMemcpyAsync(h_tail + 0, bscan + np - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_tail + 1, bflag + np - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_rb.data(), d_rb, 4 * (size_t)(nt + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  const int64_t nb = (int64_t)h_tail[0] + h_tail[1];
  const int32_t nc = h_rb[nt];
  const int64_t ns = 8 * nb;
  if (ns >= (1ll << 31))
    return fail_as(ctx, BS_ERR_RANGE, who, "more than 2^31 border states");

  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  int rounds = 0;
  int64_t total = 0;
  if (nc > 0) {
    BS_HIP(ctx, B[9].reserve(4 * nb));
    BS_HIP(ctx, B[10].reserve(4 * (int64_t)nc));
    BS_HIP(ctx, B[11].reserve(4 * ns));
    BS_HIP(ctx, B[12].reserve(ns));
    for (int k = 13; k < 19; k++)
      BS_HIP(ctx, B[k].reserve(4 * ns));
    int32_t* bpix = B[9].as<int32_t>();
    int32_t* rpix = B[10].as<int32_t>();
    int32_t* succ = B[11].as<int32_t>();
    uint8_t* kind = B[12].as<uint8_t>();
    int32_t* nxt[2] = {B[13].as<int32_t>(), B[14].as<int32_t>()};
    uint32_t* val[2] = {B[15].as<uint32_t>(), B[16].as<uint32_t>()};
    int32_t* last[2] = {B[17].as<int32_t>(), B[18].as<int32_t>()};
    lists_kernel<<<nblk(np, 256), 256, 0, st>>>(bflag, bscan, rflag, rscan, np, bpix, rpix);
    int cur = 0;
    if (ns > 0) {
      state_tiled_kernel<<<nblk(ns, 256), 256, 0, st>>>(m, d_tl, d_pb, nt, bpix, bflag, bscan, rflag, ns, succ, kind,
                                                         nxt[0], val[0], last[0]);
      int lg = 0;
      while ((1ll << lg) < ns)
        lg++;
      rounds = lg + 1;  // a list of length L <= ns closes after ceil(log2 L) rounds
      for (int it = 0; it < rounds; it++, cur ^= 1)
        jump_kernel<<<nblk(ns, 256), 256, 0, st>>>(nxt[cur], val[cur], last[cur], ns, nxt[cur ^ 1], val[cur ^ 1],
                                                    last[cur ^ 1]);
    }
    // per-contour: cnt [nc + 1] | off [nc + 1] | cstart [nc] | asum [nc] | psum [nc] | area [nc] | perim [nc]
    const int64_t n1 = (int64_t)nc + 1;
    BS_HIP(ctx, B[19].reserve(8 * (2 * n1 + 5 * (int64_t)nc)));
    int64_t* cnt = B[19].as<int64_t>();
    int64_t* off = cnt + n1;
    int32_t* cstart = reinterpret_cast<int32_t*>(off + n1);
    unsigned long long* asum = reinterpret_cast<unsigned long long*>(off + n1 + nc);
    unsigned long long* psum = asum + nc;
    double* d_area = reinterpret_cast<double*>(psum + nc);
    double* d_perim = d_area + nc;
    BS_HIP(ctx, hipMemsetAsync(cnt, 0, 8 * (2 * n1 + 5 * (int64_t)nc), st));
    contour_count_tiled_kernel<<<nblk(nc, 256), 256, 0, st>>>(m, d_tl, d_pb, nt, d_rb, rpix, nc, bscan, succ, kind,
                                                               nxt[cur], val[cur], last[cur], cnt, cstart, d_err);
    BS_HIP(ctx, cub_run(B[8], scan(cnt, off, n1)));
    int h_err = 0;
    BS_HIP(ctx, hipMemcpyAsync(&total, off + nc, 8, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    BS_HIP(ctx, hipGetLastError());
    if (h_err)
      return fail_as(ctx, BS_ERR_INTERNAL, who, "a contour list did not close within the jump-round bound");
    BS_HIP(ctx, B[20].reserve(12 * std::max<int64_t>(total, 1)));
    int32_t* xy = B[20].as<int32_t>();
    int32_t* cid = xy + 2 * total;
    BS_HIP(ctx, hipMemsetAsync(cid, 0xff, 4 * total, st));
    if (ns > 0)
      scatter_tiled_kernel<<<nblk(ns, 256), 256, 0, st>>>(d_tl, d_pb, nt, d_rb, bpix, rscan, succ, kind, nxt[cur],
                                                           val[cur], last[cur], ns, off, xy, cid, d_err);
    single_tiled_kernel<<<nblk(nc, 256), 256, 0, st>>>(d_tl, d_pb, nt, d_rb, rpix, cstart, nc, off, xy, cid);
    measure_kernel<<<nblk(total, 256), 256, 0, st>>>(xy, cid, off, total, nc, asum, psum);
    finish_kernel<<<nblk(nc, 256), 256, 0, st>>>(xy, off, nc, asum, psum, d_area, d_perim);
    BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    BS_HIP(ctx, hipGetLastError());
    if (h_err)
      return fail_as(ctx, BS_ERR_INTERNAL, who, "an emitted point fell outside its contour's range");
    out->offset = (int64_t*)malloc(8 * n1);
    out->xy = (int32_t*)malloc(8 * std::max<int64_t>(total, 1));
    out->area = (double*)malloc(8 * (size_t)nc);
    out->perimeter = (double*)malloc(8 * (size_t)nc);
    if (!out->offset || !out->xy || !out->area || !out->perimeter) {
      bs_contours_free(out);
      return fail_as(ctx, BS_ERR_NOMEM, who, "host allocation");
    }
    BS_HIP(ctx, hipMemcpyAsync(out->offset, off, 8 * n1, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->xy, xy, 8 * total, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->area, d_area, 8 * (size_t)nc, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->perimeter, d_perim, 8 * (size_t)nc, hipMemcpyDeviceToHost, st));
  } else {
    out->offset = (int64_t*)calloc(1, 8);
    if (!out->offset)
      return fail_as(ctx, BS_ERR_NOMEM, who, "host allocation");
  }
  if (d_mask)
    mask_out_tiled_kernel<<<nblk(npix, 256), 256, 0, st>>>(m, d_tl, d_ib, nt, npix, d_mask);
  BS_HIP(ctx, hipEventRecord(ev.e[5], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  out->n_contours = nc;
  out->width = 0;
  out->height = 0;
  memcpy(contour_offset, h_rb.data(), 4 * (size_t)(nt + 1));
  if (info) {
    info->ms_mask = ev.ms(0, 1);
    info->ms_close = ev.ms(1, 2);
    info->ms_label = ev.ms(2, 3);
    info->ms_trace = ev.ms(4, 5);  // (the host reads the border counts in between)
    info->ms_total = ev.ms(0, 3) + info->ms_trace;
    unsigned long long fg = 0;
    BS_HIP(ctx, hipMemcpy(&fg, d_fg, 8, hipMemcpyDeviceToHost));
    info->fg_pixels = (int64_t)fg;
    info->border_states = ns;
    info->components = nc;
    info->jump_rounds = rounds;
  }
  return BS_OK;
}

}  // namespace

extern "C" int bs_footprints_dev(bs_ctx* ctx, const double* d_image, int32_t width, int32_t height, int32_t threshold,
                                 int32_t kernel_size, int32_t iterations, uint8_t* d_mask, bs_contours* out,
                                 bs_footprint_info* info)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_image || !out || width < 1 || height < 1 || (int64_t)(width + 2ll) * (height + 2ll) >= (1ll << 31) ||
      kernel_size < 1 || kernel_size > 2 * RMAX + 1 || kernel_size % 2 == 0 || iterations < 0 || iterations > 16 ||
      threshold < 0 || threshold > 255)
    return fail(ctx, BS_ERR_INVALID, "footprints: null pointer or bad raster / threshold / kernel / iterations");
  memset(out, 0, sizeof *out);
  int32_t contour_offset[2];
  const int rc = footprints_tiles_dev(ctx, d_image, &width, &height, 1, threshold, kernel_size, iterations, d_mask, out,
                                      contour_offset, info, "footprints");
  if (rc != BS_OK)
    return rc;
  out->width = width;
  out->height = height;
  return BS_OK;
}

extern "C" int bs_footprints(bs_ctx* ctx, const double* image, int32_t width, int32_t height, int32_t threshold,
                             int32_t kernel_size, int32_t iterations, uint8_t* mask, bs_contours* out,
                             bs_footprint_info* info)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!image || !out || width < 1 || height < 1 || (int64_t)(width + 2ll) * (height + 2ll) >= (1ll << 31))
    return fail(ctx, BS_ERR_INVALID, "footprints: null pointer or bad raster size");
  const size_t npix = (size_t)width * height;
  Staging S(ctx);
  const double* d_image = S.upload(ctx->fp[FP_IN_IMAGE], image, 3 * npix);
  uint8_t* d_mask = S.room<uint8_t>(ctx->fp[FP_OUT_MASK], npix, mask != nullptr);
  if (!S.ok())
    return S.status();
  int rc = bs_footprints_dev(ctx, d_image, width, height, threshold, kernel_size, iterations, d_mask, out, info);
  if (rc != BS_OK)
    return rc;
  ContoursGuard guard{out};
  S.download(mask, d_mask, npix);
  rc = mask ? S.finish() : BS_OK;  // (without a mask nothing is in flight: the device form has waited for its own copies)
  guard.keep = rc == BS_OK;
  return rc;
}

// my_function.cpp:64-131; the GBK captions of the three header lines and the faces line are written in ASCII.
// ostream prints a float like printf("%g") of the value widened to double.
extern "C" int bs_contours_write_obj(const bs_contours* c, const char* path)
{
  if (!c || !path || c->n_contours < 0 || (c->n_contours > 0 && (!c->offset || !c->xy)) || c->width < 1 ||
      c->height < 1)
    return BS_ERR_INVALID;
  FILE* f = fopen(path, "w");
  if (!f)
    return BS_ERR_INVALID;
  fprintf(f, "# building footprints extruded to a 3-D model\n# contours: %d\n# x, y normalised to [0,1]\n\n",
          c->n_contours);
  for (int32_t i = 0; i < c->n_contours; i++)
    for (int64_t k = c->offset[i]; k < c->offset[i + 1]; k++) {
      const float x = static_cast<float>(c->xy[2 * k]) / c->width;
      const float y = 1.0f - static_cast<float>(c->xy[2 * k + 1]) / c->height;
      fprintf(f, "v %g %g 0.0\nv %g %g 1\n", (double)x, (double)y, (double)x, (double)y);
    }
  fprintf(f, "\n# faces (quads)\n");
  int64_t base = 1;
  for (int32_t i = 0; i < c->n_contours; i++) {
    const int64_t n = c->offset[i + 1] - c->offset[i];
    for (int64_t k = 0; k < n; k++) {
      const int64_t nx = (k + 1) % n;
      fprintf(f, "f %lld %lld %lld %lld\n", (long long)(base + 2 * k), (long long)(base + 2 * nx),
              (long long)(base + 2 * nx + 1), (long long)(base + 2 * k + 1));
    }
    base += 2 * n;
  }
  const bool ok = !ferror(f);
  return (fclose(f) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}

extern "C" int bs_footprints_batch_dev(bs_ctx* ctx, const double* d_image, const int32_t* width, const int32_t* height,
                                       int32_t n_tiles, int32_t threshold, int32_t kernel_size, int32_t iterations,
                                       uint8_t* d_mask, bs_contours* out, int32_t* contour_offset,
                                       bs_footprint_info* info)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (out)
    memset(out, 0, sizeof *out);
  if (!d_image || !out || !width || !height || !contour_offset || n_tiles < 1 || kernel_size < 1 ||
      kernel_size > 2 * RMAX + 1 || kernel_size % 2 == 0 || iterations < 0 || iterations > 16 || threshold < 0 ||
      threshold > 255)
    return fail(ctx, BS_ERR_INVALID, "footprints batch: null pointer, n_tiles < 1 or bad threshold / kernel / iterations");
  int64_t np = 0, npix = 0;
  for (int32_t t = 0; t < n_tiles; t++) {
    const int32_t w = width[t], h = height[t];
    if (w < 1 || h < 1 || (int64_t)(w + 2ll) * (h + 2ll) >= (1ll << 31)) {
      char msg[128];
      snprintf(msg, sizeof msg, "footprints batch: tile %d: bad raster size %d x %d", t, w, h);
      return fail(ctx, BS_ERR_INVALID, msg);
    }
    np += (int64_t)(w + 2) * (h + 2);
    npix += (int64_t)w * h;
  }
  if (npix >= (1ll << 31) - 1)
    return fail(ctx, BS_ERR_RANGE, "footprints batch: 2^31 - 1 pixels or more in all");
  if (np >= (1ll << 31))
    return fail(ctx, BS_ERR_INVALID, "footprints batch: 2^31 padded pixels or more in all");
  return footprints_tiles_dev(ctx, d_image, width, height, n_tiles, threshold, kernel_size, iterations, d_mask, out,
                              contour_offset, info, "footprints batch");
}

extern "C" int bs_footprints_batch(bs_ctx* ctx, const double* image, const int32_t* width, const int32_t* height,
                                   int32_t n_tiles, int32_t threshold, int32_t kernel_size, int32_t iterations,
                                   uint8_t* mask, bs_contours* out, int32_t* contour_offset, bs_footprint_info* info)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (out)
    memset(out, 0, sizeof *out);
  if (!image || !out || !width || !height || n_tiles < 1)
    return fail(ctx, BS_ERR_INVALID, "footprints batch: null pointer or n_tiles < 1");
  int64_t npix = 0;
  for (int32_t t = 0; t < n_tiles; t++) {
    if (width[t] < 1 || height[t] < 1) {
      char msg[128];
      snprintf(msg, sizeof msg, "footprints batch: tile %d: bad raster size %d x %d", t, width[t], height[t]);
      return fail(ctx, BS_ERR_INVALID, msg);
    }
    npix += (int64_t)width[t] * height[t];
  }
  if (npix >= (1ll << 31) - 1)
    return fail(ctx, BS_ERR_RANGE, "footprints batch: 2^31 - 1 pixels or more in all");
  Staging S(ctx);
  const double* d_image = S.upload(ctx->fp[FP_IN_IMAGE], image, 3 * (size_t)npix);
  uint8_t* d_mask = S.room<uint8_t>(ctx->fp[FP_OUT_MASK], (size_t)npix, mask != nullptr);
  if (!S.ok())
    return S.status();
  int rc = bs_footprints_batch_dev(ctx, d_image, width, height, n_tiles, threshold, kernel_size, iterations, d_mask, out,
                                   contour_offset, info);
  if (rc != BS_OK)
    return rc;
  ContoursGuard guard{out};
  S.download(mask, d_mask, (size_t)npix);
  rc = mask ? S.finish() : BS_OK;  // (without a mask nothing is in flight: the device form has waited for its own copies)
  guard.keep = rc == BS_OK;
  return rc;
}
