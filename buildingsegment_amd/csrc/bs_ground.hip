// bs_ground.hip -- ground: a terrain raster of the tile by a progressive morphological filter (DESIGN.md "Ground model"; the
// definition is written down in include/bs_api.h under "ground").
//   low       one grid-stride pass over the points: the check of the cloud, one atomicMin into low
//   K x open  per step an erosion and a dilation by the (2r+1)^2 square, separable: x pass (min), y pass (min), y pass
//             (max), x pass (max).  Every pass is van Herk / Gil-Werman: the line is cut into blocks of 2r+1, a prefix and a
//             suffix extremum inside every block, and a window is the extremum of one suffix and one prefix entry -- the cost
//             of a pass does not depend on r and no thread walks a window.
//               x pass  a workgroup takes ROW_LDS - 2r outputs of one row with r of apron each side into LDS (2 x 8 KiB); a
//                       thread scans 8 consecutive entries in registers and the carries between threads are one segmented
//                       scan of the workgroup (shuffles, 6 + 2 steps whatever r is)
//               y pass  the image is transposed by 32 x 32 tiles through LDS (loads and stores along rows), the two y passes
//                       of a step run as x passes over the transposed image, and it is transposed back.  (A thread per column
//                       and block of 2r+1 rows, walking its block down and up, was measured first: its parallelism falls with
//                       1 / r and a step at r = 255 took 7 times a step at r = 1 -- DESIGN.md has the table.)
//             EMPTY = INT32_MAX is the identity of the minimum; the maximum passes map it to INT32_MIN on load and back on
//             store, so no pass branches on it.  The flag / update of a step is fused into its last x pass; step_pixels is
//             reduced per wave, then one atomic per workgroup.  All K steps are launched without a host round trip.
//   pixels    one grid-stride pass: dtm, and the figures of the pixels
//   points    one grid-stride pass: one 4-byte gather from dtm and one byte from step; hag and class written where asked;
//             figures reduced per wave in registers, per workgroup in LDS
// Everything before the host's first wait writes scratch of the context only, so every BS_ERR_RANGE is known before an output
// is touched.  Every index is checked before it is used as an address.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>

#include "bs_common.h"
#include "bs_host.h"

namespace bs {
namespace {

// scratch of bs_ctx::gd
enum { GD_MISC, GD_LOW, GD_S, GD_T1, GD_T2, GD_STEP, GD_DTM, GD_IN_XYZ, GD_HAG, GD_CLASS, GD_COUNT };
static_assert(GD_COUNT <= (int)(sizeof(bs_ctx::gd) / sizeof(DevBuf)), "bs_ctx::gd is too short");

constexpr int GRID = BS_GROUND_GRID;        // workgroups of a pass over the points
constexpr int PIX_GRID = 2048;              // workgroups of the pass over the pixels
constexpr int ROW_LDS = BS_GROUND_ROW_LDS;  // entries of a row segment in LDS: 256 threads x ITEMS
constexpr int ITEMS = ROW_LDS / 256;
constexpr int MAX_STEPS = BS_GROUND_MAX_STEPS;
constexpr int MAX_RADIUS = BS_GROUND_MAX_RADIUS;
constexpr int32_t COORD_LIMIT = 1 << 23;
constexpr int32_t EMPTY = INT32_MAX;
static_assert(ITEMS == 8 && ROW_LDS - 2 * MAX_RADIUS >= 1024, "the x pass scans 8 entries a thread");
enum { R_XY = 1, R_COORD = 2 };  // the bits of the range word

// the 64-bit words of GD_MISC
enum { M_RANGE, M_STEP, M_GROUND_PIX = M_STEP + MAX_STEPS, M_OBJECT_PIX, M_EMPTY_PIX, M_FILLED_PIX, M_GROUND_PTS, M_LOW_PTS,
       M_OBJECT_PTS, M_SUM_HAG, M_DTM_MIN, M_DTM_MAX, M_HAG_MIN, M_HAG_MAX, M_WORDS };

// minimum, or maximum with EMPTY below everything
template <bool MAX>
struct Op {
  static constexpr int32_t ID = MAX ? INT32_MIN : INT32_MAX;
  __device__ static int32_t in(int32_t v) { return MAX && v == EMPTY ? INT32_MIN : v; }
  __device__ static int32_t out(int32_t v) { return MAX && v == INT32_MIN ? EMPTY : v; }
  __device__ static int32_t f(int32_t a, int32_t b) { return MAX ? max(a, b) : min(a, b); }
};

__global__ __launch_bounds__(256) void gd_init_kernel(unsigned long long* __restrict__ words)
{
  const int k = threadIdx.x;
  if (k >= M_WORDS)
    return;
  long long v = 0;
  if (k == M_DTM_MIN || k == M_HAG_MIN)
    v = INT32_MAX;
  if (k == M_DTM_MAX || k == M_HAG_MAX)
    v = INT32_MIN;
  words[k] = (unsigned long long)v;
}

__global__ __launch_bounds__(256) void gd_fill_kernel(int32_t* __restrict__ low, long long npix)
{
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x)
    low[p] = EMPTY;
}

// ---- 1. low ---------------------------------------------------------------------------------------------------------------
// the range bits of a point and its pixel
__device__ inline int point_pixel(const int32_t* __restrict__ xyz, unsigned i, int32_t cell, int32_t w, int32_t h, unsigned* p,
                                  int32_t* z)
{
  const int32_t x = xyz[3 * i], y = xyz[3 * i + 1];
  *z = xyz[3 * i + 2];
  const int32_t bx = x / cell, by = y / cell;
  int mine = 0;
  if (x < 0 || y < 0 || bx >= w || by >= h)
    mine |= R_XY;
  if (x >= COORD_LIMIT || y >= COORD_LIMIT || *z >= COORD_LIMIT || x <= -COORD_LIMIT || y <= -COORD_LIMIT || *z <= -COORD_LIMIT)
    mine |= R_COORD;
  *p = mine ? 0u : (unsigned)by * (unsigned)w + (unsigned)bx;
  return mine;
}

__global__ __launch_bounds__(256) void gd_low_kernel(const int32_t* __restrict__ xyz, long long n, int32_t cell, int32_t w,
                                                     int32_t h, int32_t* __restrict__ low, unsigned long long* __restrict__ words)
{
  int bad = 0;
  // (n < 2^29: 3 i fits 32 bits, and so does a pixel's number)
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n; i += gridDim.x * blockDim.x) {
    unsigned p;
    int32_t z;
    const int mine = point_pixel(xyz, i, cell, w, h, &p, &z);
    bad |= mine;
    // (low only falls: whatever a plain read returns is no lower than the pixel's minimum now, so a point that is not below it
    // cannot change it -- most points of a full pixel skip the atomic)
    if (!mine && z < *(volatile const int32_t*)(low + p))
      atomicMin(low + p, z);
  }
  if (bad)
    atomicOr(words + M_RANGE, (unsigned long long)bad);
}

__global__ __launch_bounds__(256) void gd_start_kernel(const int32_t* __restrict__ low, long long npix, int32_t* __restrict__ S,
                                                       uint8_t* __restrict__ step)
{
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
    const int32_t l = low[p];
    S[p] = l;
    step[p] = l == EMPTY ? 255 : 0;
  }
}

// ---- 2. open: x pass ------------------------------------------------------------------------------------------------------
// Prefix extrema inside the blocks of a line of ROW_LDS entries, 8 consecutive entries a thread: v[e] in, the prefix out.
// start[e]: entry e of this thread opens a block.  Thread 0's first entry opens one.  Every thread of the workgroup calls this.
template <bool MAX>
__device__ inline void block_prefix(int32_t (&v)[ITEMS], const bool (&start)[ITEMS], int32_t* s_wave_v, int* s_wave_f)
{
  using O = Op<MAX>;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int first = ITEMS;  // the first entry that opens a block
  int32_t run = O::ID;
#pragma unroll
  for (int e = 0; e < ITEMS; e++) {
    if (start[e]) {
      run = O::ID;
      if (first == ITEMS)
        first = e;
    }
    run = O::f(run, v[e]);
    v[e] = run;
  }
  // inclusive segmented scan of (flag, run) over the wave: (fa, a) then (fb, b) = (fa | fb, fb ? b : f(a, b))
  int f = first < ITEMS;
  int32_t a = run;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t pa = __shfl_up(a, d);
    const int pf = __shfl_up(f, d);
    if (lane >= d) {
      if (!f)
        a = O::f(pa, a);
      f |= pf;
    }
  }
  if (lane == 63) {
    s_wave_v[wv] = a;
    s_wave_f[wv] = f;
  }
  __syncthreads();
  // what reaches this thread from the threads before it: the waves before, then the lanes before
  int32_t carry = O::ID;
  for (int k = 0; k < wv; k++)
    carry = s_wave_f[k] ? s_wave_v[k] : O::f(carry, s_wave_v[k]);
  const int32_t la = __shfl_up(a, 1);
  const int lf = __shfl_up(f, 1);
  if (lane > 0)
    carry = lf ? la : O::f(carry, la);
#pragma unroll
  for (int e = 0; e < ITEMS; e++)
    if (e < first)
      v[e] = O::f(carry, v[e]);
  __syncthreads();  // (s_wave_* may be written again)
}

// One x pass over every row segment: out[y][x] = the extremum of in[y][x - r .. x + r] clipped to the row.  FLAG (the last
// pass of a step, MAX): `out` is S, read as S_{k-1} and written as S_k = O_k at the same pixels; the pixels with step == 0,
// S_{k-1} != EMPTY and S_{k-1} - O_k > t get step = k and are counted.
template <bool MAX, bool FLAG>
__global__ __launch_bounds__(256) void gd_xpass_kernel(const int32_t* __restrict__ in, int32_t w, int32_t h, int32_t r,
                                                       long long n_seg, int32_t seg_per_row, int32_t* __restrict__ out,
                                                       uint8_t* __restrict__ step, int32_t k, int32_t t,
                                                       unsigned long long* __restrict__ count)
{
  using O = Op<MAX>;
  __shared__ __attribute__((aligned(16))) int32_t s_g[ROW_LDS], s_h[ROW_LDS];
  __shared__ int32_t s_wave_v[4];
  __shared__ int s_wave_f[4];
  __shared__ unsigned s_flagged;
  const int win = 2 * r + 1, tx = ROW_LDS - 2 * r;  // outputs of a segment
  if (FLAG) {
    if (threadIdx.x == 0)
      s_flagged = 0;
    __syncthreads();
  }
  unsigned flagged = 0;
  for (long long seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
    const int32_t y = (int32_t)(seg / seg_per_row);
    const int32_t x0 = (int32_t)(seg - (long long)y * seg_per_row) * tx;
    const int32_t* __restrict__ row = in + (long long)y * w;
    // entry j of the line is x0 - r + j; outside the row: the identity
    for (int j = threadIdx.x; j < ROW_LDS; j += 256) {
      const long long x = (long long)x0 - r + j;
      s_g[j] = (x >= 0 && x < w) ? O::in(row[x]) : O::ID;
    }
    __syncthreads();
    int32_t a[ITEMS], b[ITEMS];
    bool sa[ITEMS], sb[ITEMS];
    const int base = threadIdx.x * ITEMS;
#pragma unroll
    for (int e = 0; e < ITEMS; e++) {
      a[e] = s_g[base + e];                  // forward: entry base + e, a block opens at a multiple of win
      b[e] = s_g[ROW_LDS - 1 - base - e];    // backward: the line reversed, a block opens at the last entry of a block
      sa[e] = (base + e) % win == 0;
      sb[e] = (ROW_LDS - 1 - base - e) % win == win - 1 || base + e == 0;
    }
    __syncthreads();
    block_prefix<MAX>(a, sa, s_wave_v, s_wave_f);
    block_prefix<MAX>(b, sb, s_wave_v, s_wave_f);
#pragma unroll
    for (int e = 0; e < ITEMS; e++) {
      s_g[base + e] = a[e];
      s_h[ROW_LDS - 1 - base - e] = b[e];
    }
    __syncthreads();
    int32_t* __restrict__ orow = out + (long long)y * w;
    for (int i = threadIdx.x; i < tx; i += 256) {
      const long long x = (long long)x0 + i;
      if (x >= w)
        break;
      const int32_t o = O::out(O::f(s_h[i], s_g[i + 2 * r]));
      if (FLAG) {
        const int32_t s = orow[x];
        const long long p = (long long)y * w + x;
        if (s != EMPTY && step[p] == 0 && (long long)s - (long long)o > (long long)t) {
          step[p] = (uint8_t)k;
          flagged++;
        }
      }
      orow[x] = o;
    }
    __syncthreads();  // (the line is loaded again)
  }
  if (FLAG) {
    for (int o = 32; o > 0; o >>= 1)
      flagged += __shfl_xor(flagged, o);
    if ((threadIdx.x & 63) == 0 && flagged)
      atomicAdd(&s_flagged, flagged);
    __syncthreads();
    if (threadIdx.x == 0 && s_flagged)
      atomicAdd(count, (unsigned long long)s_flagged);
  }
}

// ---- 2. open: y pass ------------------------------------------------------------------------------------------------------
// out [w][h] = in [h][w] transposed, by 32 x 32 tiles through LDS: loads and stores both run along a row.  The two y passes of
// a step are x passes over the transposed image.
__global__ __launch_bounds__(256) void gd_transpose_kernel(const int32_t* __restrict__ in, int32_t w, int32_t h,
                                                           long long n_tiles, int32_t tiles_x, int32_t* __restrict__ out)
{
  __shared__ int32_t s_t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long long tyi = t / tiles_x;
    const int32_t x0 = (int32_t)(t - tyi * tiles_x) * 32, y0 = (int32_t)tyi * 32;
    for (int j = ty; j < 32; j += 8)
      if (x0 + tx < w && y0 + j < h)
        s_t[j][tx] = in[(long long)(y0 + j) * w + x0 + tx];
    __syncthreads();
    for (int j = ty; j < 32; j += 8)
      if (y0 + tx < h && x0 + j < w)
        out[(long long)(x0 + j) * h + y0 + tx] = s_t[tx][j];
    __syncthreads();
  }
}

// ---- 3. pixels ------------------------------------------------------------------------------------------------------------
__device__ inline void wave_sum(unsigned long long& v)
{
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_xor(v, o);
}

__global__ __launch_bounds__(256) void gd_pixels_kernel(const int32_t* __restrict__ low, const int32_t* __restrict__ S,
                                                        const uint8_t* __restrict__ step, long long npix,
                                                        int32_t* __restrict__ dtm, unsigned long long* __restrict__ words)
{
  __shared__ unsigned long long s_cnt[4];
  __shared__ int32_t s_mn, s_mx;
  if (threadIdx.x < 4)
    s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    s_mn = INT32_MAX;
    s_mx = INT32_MIN;
  }
  __syncthreads();
  unsigned long long c[4] = {0, 0, 0, 0};  // ground, object, empty, filled
  int32_t mn = INT32_MAX, mx = INT32_MIN;
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
    const int32_t l = low[p];
    const unsigned st = step[p];
    const int32_t d = st == 0 ? l : S[p];
    dtm[p] = d;
    c[0] += st == 0;
    c[1] += st != 0 && st != 255;
    c[2] += l == EMPTY;
    c[3] += l == EMPTY && d != EMPTY;
    if (d != EMPTY) {
      mn = min(mn, d);
      mx = max(mx, d);
    }
  }
  for (int j = 0; j < 4; j++)
    wave_sum(c[j]);
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o));
    mx = max(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    for (int j = 0; j < 4; j++)
      if (c[j])
        atomicAdd(&s_cnt[j], c[j]);
    atomicMin(&s_mn, mn);
    atomicMax(&s_mx, mx);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x])
    atomicAdd(words + M_GROUND_PIX + threadIdx.x, s_cnt[threadIdx.x]);
  if (threadIdx.x == 0 && s_mn <= s_mx) {
    atomicMin(reinterpret_cast<long long*>(words) + M_DTM_MIN, (long long)s_mn);
    atomicMax(reinterpret_cast<long long*>(words) + M_DTM_MAX, (long long)s_mx);
  }
}
static_assert(M_OBJECT_PIX == M_GROUND_PIX + 1 && M_EMPTY_PIX == M_GROUND_PIX + 2 && M_FILLED_PIX == M_GROUND_PIX + 3,
              "gd_pixels_kernel adds its four counts in this order");

// ---- 4. points ------------------------------------------------------------------------------------------------------------
// (the cloud has passed its check: every pixel is inside the lattice)
__global__ __launch_bounds__(256) void gd_points_kernel(const int32_t* __restrict__ xyz, long long n, int32_t cell, int32_t w,
                                                        int32_t h, const int32_t* __restrict__ dtm,
                                                        const uint8_t* __restrict__ step, int32_t tol, int32_t min_height,
                                                        int32_t* __restrict__ hag_out, uint8_t* __restrict__ class_out,
                                                        unsigned long long* __restrict__ words)
{
  __shared__ unsigned long long s_cnt[4];  // ground, low, object points; the sum of hag over the ground (two's complement)
  __shared__ int32_t s_mn, s_mx;
  if (threadIdx.x < 4)
    s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    s_mn = INT32_MAX;
    s_mx = INT32_MIN;
  }
  __syncthreads();
  unsigned long long c[4] = {0, 0, 0, 0};
  int32_t mn = INT32_MAX, mx = INT32_MIN;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n; i += gridDim.x * blockDim.x) {
    unsigned p;
    int32_t z;
    if (point_pixel(xyz, i, cell, w, h, &p, &z))
      continue;  // (cannot happen behind the check; stay in bounds)
    const int32_t d = dtm[p];
    const unsigned st = step[p];
    // (a pixel with a point has a dtm; |z| and |dtm| < 2^23: the difference fits)
    const int32_t hg = d == EMPTY ? 0 : z - d;
    const int cl = (st == 0 && hg <= tol) ? 0 : (hg >= min_height ? 2 : 1);
    if (hag_out)
      hag_out[i] = hg;
    if (class_out)
      class_out[i] = (uint8_t)cl;
    c[0] += cl == 0;
    c[1] += cl == 1;
    c[2] += cl == 2;
    if (cl == 0)
      c[3] += (unsigned long long)(long long)hg;
    mn = min(mn, hg);
    mx = max(mx, hg);
  }
  for (int j = 0; j < 4; j++)
    wave_sum(c[j]);
  for (int o = 32; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o));
    mx = max(mx, __shfl_xor(mx, o));
  }
  if ((threadIdx.x & 63) == 0) {
    for (int j = 0; j < 4; j++)
      if (c[j])
        atomicAdd(&s_cnt[j], c[j]);
    atomicMin(&s_mn, mn);
    atomicMax(&s_mx, mx);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_cnt[threadIdx.x])
    atomicAdd(words + M_GROUND_PTS + threadIdx.x, s_cnt[threadIdx.x]);
  if (threadIdx.x == 0 && s_mn <= s_mx) {
    atomicMin(reinterpret_cast<long long*>(words) + M_HAG_MIN, (long long)s_mn);
    atomicMax(reinterpret_cast<long long*>(words) + M_HAG_MAX, (long long)s_mx);
  }
}
static_assert(M_LOW_PTS == M_GROUND_PTS + 1 && M_OBJECT_PTS == M_GROUND_PTS + 2 && M_SUM_HAG == M_GROUND_PTS + 3,
              "gd_points_kernel adds its four figures in this order");

// ---- host -----------------------------------------------------------------------------------------------------------------
int check_args(bs_ctx* ctx, const void* xyz, int64_t n, const int32_t* extent, const struct bs_ground_params* q, const void* out,
               int32_t* width, int32_t* height, int32_t* threshold)
{
  if (!xyz || !extent || !q || !out)
    return fail(ctx, BS_ERR_INVALID, "ground: null pointer");
  if (n < 1 || q->cell < 1)
    return fail(ctx, BS_ERR_INVALID, "ground: n < 1 or cell < 1");
  if (bs_grid_dims(extent, q->cell, width, height) != BS_OK)
    return fail(ctx, BS_ERR_INVALID, "ground: bad extent");
  if (q->n_steps < 1 || q->n_steps > MAX_STEPS)
    return fail(ctx, BS_ERR_INVALID, "ground: n_steps outside 1 .. 16");
  for (int k = 0; k < q->n_steps; k++)
    if (q->radius[k] < 1 || q->radius[k] > MAX_RADIUS || (k > 0 && q->radius[k] <= q->radius[k - 1]))
      return fail(ctx, BS_ERR_INVALID, "ground: a radius outside 1 .. 255, or radii that do not increase");
  if (q->s_num < 0 || q->s_den < 1)
    return fail(ctx, BS_ERR_INVALID, "ground: the slope needs s_num >= 0 and s_den >= 1");
  if (q->dh0 < 0 || q->dh_max < 0 || q->tol < 0 || q->min_height < 0)
    return fail(ctx, BS_ERR_INVALID, "ground: a negative dh0, dh_max, tol or min_height");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "ground: 2^29 points or more");
  if ((long long)*width * *height >= (1ll << 31) - 1)
    return fail(ctx, BS_ERR_RANGE, "ground: 2^31 - 1 pixels or more");
  for (int k = 0; k < q->n_steps; k++) {
    // s_num * (r_k - r_{k-1}) * cell < 2^31 * 2^8 * 2^31: beyond 64 bits
    const __int128 rise = (__int128)q->s_num * (q->radius[k] - (k ? q->radius[k - 1] : 0)) * q->cell / q->s_den;
    const __int128 t = (__int128)q->dh0 + rise;
    threshold[k] = t > (__int128)q->dh_max ? q->dh_max : (int32_t)t;
  }
  return BS_OK;
}

int pix_grid(long long npix) { return (int)std::max<long long>(1, std::min<long long>(nblk(npix, 256), PIX_GRID)); }

// the stage on a device cloud; res is zeroed; every output may be NULL (the scratch images of the context hold low, dtm and
// step in any case: the host-memory twin copies from there)
int ground(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t width, int32_t height, const struct bs_ground_params& q,
           const int32_t* threshold, int32_t* d_low, int32_t* d_dtm, uint8_t* d_step, int32_t* d_hag, uint8_t* d_class,
           struct bs_ground& res)
{
  const long long npix = (long long)width * height;
  const size_t np = (size_t)npix;
  const int K = q.n_steps;
  res.width = width;
  res.height = height;
  res.cell = q.cell;
  res.n_steps = K;
  res.grid = GRID;
  res.row_lds = ROW_LDS;
  res.n_points = n;
  for (int k = 0; k < K; k++) {
    res.radius[k] = q.radius[k];
    res.threshold[k] = threshold[k];
  }
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->gd;
  Events<4 + MAX_STEPS> ev;
  for (int i = 0; i < 4 + K; i++)
    BS_HIP(ctx, hipEventCreate(&ev.e[i]));
  BS_HIP(ctx, B[GD_MISC].reserve(8 * M_WORDS));
  for (int b : {GD_LOW, GD_S, GD_T1, GD_T2, GD_DTM})
    BS_HIP(ctx, B[b].reserve(4 * np));
  BS_HIP(ctx, B[GD_STEP].reserve(np));
  unsigned long long* words = B[GD_MISC].as<unsigned long long>();
  int32_t* low = B[GD_LOW].as<int32_t>();
  int32_t* S = B[GD_S].as<int32_t>();
  int32_t* T1 = B[GD_T1].as<int32_t>();
  int32_t* T2 = B[GD_T2].as<int32_t>();
  int32_t* dtm = B[GD_DTM].as<int32_t>();
  uint8_t* step = B[GD_STEP].as<uint8_t>();
  unsigned long long h_words[M_WORDS] = {};
  const int pgrid = pix_grid(npix);
  const int ngrid = (int)std::max<long long>(1, std::min<long long>(nblk(n, 256), GRID));

  // 1. low
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  gd_init_kernel<<<1, 256, 0, st>>>(words);
  gd_fill_kernel<<<pgrid, 256, 0, st>>>(low, npix);
  gd_low_kernel<<<ngrid, 256, 0, st>>>(d_xyz, n, q.cell, width, height, low, words);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  // 2. open
  gd_start_kernel<<<pgrid, 256, 0, st>>>(low, npix, S, step);
  for (int k = 1; k <= K; k++) {
    const int32_t r = q.radius[k - 1];
    const int32_t seg_per_row = (width + (ROW_LDS - 2 * r) - 1) / (ROW_LDS - 2 * r);
    const long long n_seg = (long long)seg_per_row * height;
    const int xgrid = (int)std::min<long long>(n_seg, 1 << 16);
    // the same for the transposed image: rows of `height` entries, `width` of them
    const int32_t tseg_per_row = (height + (ROW_LDS - 2 * r) - 1) / (ROW_LDS - 2 * r);
    const long long tn_seg = (long long)tseg_per_row * width;
    const int tgrid = (int)std::min<long long>(tn_seg, 1 << 16);
    const int32_t tiles_x = (width + 31) / 32, tiles_y = (height + 31) / 32;
    const long long n_tiles = (long long)tiles_x * tiles_y, n_tiles_t = n_tiles;
    const int trgrid = (int)std::min<long long>(n_tiles, 1 << 16);
    gd_xpass_kernel<false, false><<<xgrid, 256, 0, st>>>(S, width, height, r, n_seg, seg_per_row, T1, nullptr, 0, 0, nullptr);
    gd_transpose_kernel<<<trgrid, 256, 0, st>>>(T1, width, height, n_tiles, tiles_x, T2);
    gd_xpass_kernel<false, false><<<tgrid, 256, 0, st>>>(T2, height, width, r, tn_seg, tseg_per_row, T1, nullptr, 0, 0, nullptr);  // E
    gd_xpass_kernel<true, false><<<tgrid, 256, 0, st>>>(T1, height, width, r, tn_seg, tseg_per_row, T2, nullptr, 0, 0, nullptr);
    gd_transpose_kernel<<<trgrid, 256, 0, st>>>(T2, height, width, n_tiles_t, tiles_y, T1);
    gd_xpass_kernel<true, true><<<xgrid, 256, 0, st>>>(T1, width, height, r, n_seg, seg_per_row, S, step, k, threshold[k - 1],
                                                       words + M_STEP + k - 1);
    BS_HIP(ctx, hipEventRecord(ev.e[1 + k], st));
  }
  // 3. pixels
  gd_pixels_kernel<<<pgrid, 256, 0, st>>>(low, S, step, npix, dtm, words);
  BS_HIP(ctx, hipMemcpyAsync(h_words, words, 8, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipEventRecord(ev.e[2 + K], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the range flags, before anything of the caller's is written
  BS_HIP(ctx, hipGetLastError());
  if (h_words[M_RANGE] & R_XY)
    return fail(ctx, BS_ERR_RANGE, "ground: a point with a negative x or y, or whose pixel lies outside the lattice");
  if (h_words[M_RANGE])
    return fail(ctx, BS_ERR_RANGE, "ground: a coordinate at or beyond 2^23");
  // 4. points
  gd_points_kernel<<<ngrid, 256, 0, st>>>(d_xyz, n, q.cell, width, height, dtm, step, q.tol, q.min_height, d_hag, d_class, words);
  BS_HIP(ctx, hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, st));
  if (d_low)
    BS_HIP(ctx, hipMemcpyAsync(d_low, low, 4 * np, hipMemcpyDeviceToDevice, st));
  if (d_dtm)
    BS_HIP(ctx, hipMemcpyAsync(d_dtm, dtm, 4 * np, hipMemcpyDeviceToDevice, st));
  if (d_step)
    BS_HIP(ctx, hipMemcpyAsync(d_step, step, np, hipMemcpyDeviceToDevice, st));
  BS_HIP(ctx, hipEventRecord(ev.e[3 + K], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  for (int k = 0; k < K; k++) {
    res.step_pixels[k] = (int64_t)h_words[M_STEP + k];
    res.ms_step[k] = ev.ms(1 + k, 2 + k);
  }
  res.n_ground_pixels = (int64_t)h_words[M_GROUND_PIX];
  res.n_object_pixels = (int64_t)h_words[M_OBJECT_PIX];
  res.n_empty_pixels = (int64_t)h_words[M_EMPTY_PIX];
  res.n_filled_pixels = (int64_t)h_words[M_FILLED_PIX];
  res.n_ground_points = (int64_t)h_words[M_GROUND_PTS];
  res.n_low_points = (int64_t)h_words[M_LOW_PTS];
  res.n_object_points = (int64_t)h_words[M_OBJECT_PTS];
  res.sum_hag_ground = (int64_t)h_words[M_SUM_HAG];
  res.dtm_min = (int32_t)(int64_t)h_words[M_DTM_MIN];
  res.dtm_max = (int32_t)(int64_t)h_words[M_DTM_MAX];
  res.hag_min = (int32_t)(int64_t)h_words[M_HAG_MIN];
  res.hag_max = (int32_t)(int64_t)h_words[M_HAG_MAX];
  res.ms_low = ev.ms(0, 1);
  res.ms_open = ev.ms(1, 2 + K);
  res.ms_points = ev.ms(2 + K, 3 + K);
  return BS_OK;
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_ground_free(struct bs_ground* g)
{
  if (g)
    memset(g, 0, sizeof *g);
}

extern "C" int bs_ground_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* extent,
                             const struct bs_ground_params* params, int32_t* d_low, int32_t* d_dtm, uint8_t* d_step,
                             int32_t* d_hag, uint8_t* d_class, struct bs_ground* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int32_t width = 0, height = 0, threshold[MAX_STEPS] = {};
  int rc = check_args(ctx, d_xyz, n, extent, params, out, &width, &height, threshold);
  if (rc != BS_OK)
    return rc;
  struct bs_ground res;
  memset(&res, 0, sizeof res);
  rc = ground(ctx, d_xyz, n, width, height, *params, threshold, d_low, d_dtm, d_step, d_hag, d_class, res);
  if (rc != BS_OK)
    return rc;
  *out = res;
  return BS_OK;
}

extern "C" int bs_ground(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* extent, const struct bs_ground_params* params,
                         int32_t* low, int32_t* dtm, uint8_t* step, int32_t* hag, uint8_t* cls, struct bs_ground* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int32_t width = 0, height = 0, threshold[MAX_STEPS] = {};
  int rc = check_args(ctx, xyz, n, extent, params, out, &width, &height, threshold);
  if (rc != BS_OK)
    return rc;
  struct bs_ground res;
  memset(&res, 0, sizeof res);
  DevBuf* B = ctx->gd;
  const size_t np = (size_t)width * (size_t)height, nn = (size_t)n;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(B[GD_IN_XYZ], xyz, 3 * nn);
  int32_t* d_hag = S.room<int32_t>(B[GD_HAG], nn, hag != nullptr);
  uint8_t* d_class = S.room<uint8_t>(B[GD_CLASS], nn, cls != nullptr);
  if (!S.ok())
    return S.status();
  rc = ground(ctx, d_xyz, n, width, height, *params, threshold, nullptr, nullptr, nullptr, d_hag, d_class, res);
  if (rc != BS_OK)
    return rc;
  S.download(low, B[GD_LOW].as<int32_t>(), np);
  S.download(dtm, B[GD_DTM].as<int32_t>(), np);
  S.download(step, B[GD_STEP].as<uint8_t>(), np);
  S.download(hag, d_hag, nn);
  S.download(cls, d_class, nn);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  *out = res;
  return BS_OK;
}
