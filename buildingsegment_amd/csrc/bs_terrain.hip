// bs_terrain.hip -- terrain: the ground height of every building from the points around it (DESIGN.md "Terrain"; the
// definition is written down in include/bs_api.h under "terrain").
//   ring      over the image alone, never the cloud: owner = map, the first frontier (the building pixels with an outside
//             4-neighbour), then `ring` rounds of a push and a commit kernel over frontier worklists as the roof fill has them,
//             all launched without a host round trip; a kernel leaves at once on an empty list.  Besides owner and dist the
//             commit writes the ring image: the owner on ring pixels, -1 everywhere else
//   points    one grid-stride pass: the check of the cloud, one 4-byte gather from the ring image, ring_points counted a
//             building of the wave at a time before any atomic, and one atomicMin into low for the points on ring pixels alone
//   pixels    one grid-stride pass: the keys (building << 32) | (low ^ 0x80000000) of the ring pixels that hold a point,
//             compacted; the per-building figures reduced in registers per wave, then in LDS below FIG_CAP and by global
//             atomics above
//   pick      one radix sort of the keys over the bits in use, one exclusive sum of ground_pixels, one thread per building
// Everything before the host's first wait writes scratch of the context only, so every BS_ERR_RANGE is known before an output
// is touched.  Every index read from memory is checked before it is used as an address.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_common.h"
#include "bs_host.h"

namespace bs {
namespace {

// scratch of bs_ctx::tn
enum { TN_MISC, TN_OWNER, TN_RING, TN_NEXT, TN_DIST, TN_LOW, TN_LIST_A, TN_LIST_B, TN_KEYS, TN_SORTED, TN_TMP, TN_FIG, TN_OFF,
       TN_IN_XYZ, TN_IN_MAP, TN_COUNT };
static_assert(TN_COUNT <= (int)(sizeof(bs_ctx::tn) / sizeof(DevBuf)), "bs_ctx::tn is too short");

constexpr int FIG_CAP = BS_TERRAIN_FIG_CAP;  // buildings 0 .. FIG_CAP - 1: figures reduced in LDS (24 KiB in tn_pixels_kernel)
constexpr int GRID = BS_TERRAIN_GRID;        // workgroups of the pass over the points: eight of them share a CU
constexpr int PIX_GRID = 2048;               // workgroups of the pass over the pixels
constexpr int RING_GRID = 512;               // workgroups of a ring kernel (grid-stride over the list)
constexpr int MAX_RING = BS_TERRAIN_MAX_RING;
constexpr int32_t COORD_LIMIT = 1 << 23;
// the int words of TN_MISC; behind them the list counts: round r reads W_CNT + r - 1 and fills W_CNT + r
enum { W_RANGE, W_ERR, W_ROUNDS, W_NKEYS, W_CNT, W_WORDS = W_CNT + MAX_RING + 1 };
enum { R_XY = 1, R_COORD = 2, R_MAP = 4 };  // the bits of W_RANGE
enum { E_PICK = 1 };                        // the bits of W_ERR
// the arrays of TN_FIG: four of 64 bits, then four of 32
enum { F_RING_PIXELS, F_GROUND_PIXELS, F_RING_POINTS, F_SUM, F_WIDE };
enum { G_MIN, G_MAX, G_GROUND, G_STATUS, G_NARROW };

struct Fig {  // per building, device: array j starts j * stride entries behind its base
  unsigned long long* wide;
  int32_t* narrow;
  long long stride;
  __device__ unsigned long long* w(int j, int32_t c) const { return wide + j * stride + c; }
  __device__ int32_t* n(int j, int32_t c) const { return narrow + j * stride + c; }
};

// append v of the lanes with `take` to list[*count ...]: one atomicAdd per wave (every lane of the wave calls this)
template <class T>
__device__ inline void wave_append(bool take, T v, T* __restrict__ list, int32_t* __restrict__ count)
{
  const unsigned long long m = __ballot(take);
  if (!m)
    return;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  int32_t base = 0;
  if (lane == leader)
    base = atomicAdd(count, (int32_t)__popcll(m));
  base = __shfl(base, leader);
  if (take)
    list[base + __popcll(m & ((1ull << lane) - 1))] = v;
}

// the same for a whole workgroup of 256 threads: one atomicAdd per workgroup (every thread calls this, once per kernel)
__device__ inline void block_append(bool take, int32_t v, int32_t* __restrict__ list, int32_t* __restrict__ count)
{
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(take);
  if (lane == 0)
    s_wave[wv] = (int)__popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = tot ? atomicAdd(count, tot) : 0;
  }
  __syncthreads();
  if (take) {
    int off = s_base;
    for (int k = 0; k < wv; k++)
      off += s_wave[k];
    list[off + __popcll(m & ((1ull << lane) - 1))] = v;
  }
}

// ---- 1. ring --------------------------------------------------------------------------------------------------------------
// owner_0, the cleared images, the check of the map, and the first frontier: the building pixels with an outside 4-neighbour
__global__ __launch_bounds__(256) void tn_init_kernel(const int32_t* __restrict__ map, int w, int h, int32_t nb,
                                                      int32_t* __restrict__ owner, int32_t* __restrict__ ringimg,
                                                      int32_t* __restrict__ next, uint8_t* __restrict__ dist,
                                                      int32_t* __restrict__ low, int32_t* __restrict__ list,
                                                      int* __restrict__ words)
{
  const int64_t npix = (int64_t)w * h, i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool front = false;
  if (i < npix) {
    const int32_t m = map[i], o = m < 0 ? -1 : m;
    if (m >= nb)
      atomicOr(words + W_RANGE, R_MAP);
    owner[i] = o;
    ringimg[i] = -1;
    next[i] = INT32_MAX;
    dist[i] = 0;
    low[i] = INT32_MAX;
    if (o >= 0) {
      const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
      front = (x > 0 && map[i - 1] < 0) || (x < w - 1 && map[i + 1] < 0) || (y > 0 && map[i - w] < 0) ||
              (y < h - 1 && map[i + w] < 0);
    }
  }
  block_append(front, (int32_t)i, list, words + W_CNT);
}

// One round, first half: the pixels of `cur` (labelled in the round before; in round 1 the first frontier) push their owner
// to their unlabelled 4-neighbours.  owner is only read here: whatever this round labels is written by the commit.
__global__ __launch_bounds__(256) void tn_push_kernel(const int32_t* __restrict__ owner, int w, int h,
                                                      const int32_t* __restrict__ cur, const int32_t* __restrict__ n_cur,
                                                      int32_t* __restrict__ next, int32_t* __restrict__ out,
                                                      int32_t* __restrict__ n_out)
{
  const int64_t cnt = *n_cur;
  if (cnt == 0)
    return;
  const int64_t cnt64 = (cnt + 63) & ~(int64_t)63, stride = (int64_t)gridDim.x * blockDim.x;  // whole waves stay together
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < cnt64; t += stride) {
    int32_t pix = -1, o = 0;
    int x = 0, y = 0;
    if (t < cnt) {
      pix = cur[t];
      o = owner[pix];
      y = pix / w;
      x = pix - y * w;
    }
    for (int d = 0; d < 4; d++) {
      const int nx = x + (d == 0) - (d == 1), ny = y + (d == 2) - (d == 3);
      bool won = false;
      int32_t q = 0;
      if (pix >= 0 && o >= 0 && nx >= 0 && nx < w && ny >= 0 && ny < h) {
        q = ny * w + nx;
        if (owner[q] == -1)
          won = atomicMin(next + q, o) == INT32_MAX;  // the first pusher lists the pixel
      }
      wave_append(won, q, out, n_out);
    }
  }
}

// One round, second half: the pixels the round reached take the smallest owner that was pushed to them.
__global__ __launch_bounds__(256) void tn_commit_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ n_list,
                                                        const int32_t* __restrict__ next, int round, int32_t* __restrict__ owner,
                                                        int32_t* __restrict__ ringimg, uint8_t* __restrict__ dist,
                                                        int* __restrict__ rounds)
{
  const int64_t cnt = *n_list;
  if (cnt == 0)
    return;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t t = first; t < cnt; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t q = list[t], o = next[q];
    owner[q] = o;
    ringimg[q] = o;
    dist[q] = (uint8_t)round;
  }
  if (first == 0)
    *rounds += 1;  // (one writer: the kernels of a stream run one after the other)
}

// ---- 2. points ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tn_fig_init_kernel(Fig f, int32_t nb)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb)
    return;
  for (int j = 0; j < F_WIDE; j++)
    *f.w(j, c) = 0;
  *f.n(G_MIN, c) = INT32_MAX;
  *f.n(G_MAX, c) = INT32_MIN;
  *f.n(G_GROUND, c) = 0;
  *f.n(G_STATUS, c) = 0;
}

__global__ __launch_bounds__(256, 8) void tn_points_kernel(const int32_t* __restrict__ xyz, long long n, int32_t bin, int32_t w,
                                                           int32_t h, int32_t nb, const int32_t* __restrict__ ringimg,
                                                           int32_t* __restrict__ low, Fig f, int* __restrict__ words)
{
  __shared__ unsigned s_points[FIG_CAP];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x)
    s_points[k] = 0;
  __syncthreads();
  int bad = 0;
  // (n < 2^29: 3 i fits 32 bits, and so does a pixel's number)
  const unsigned n64 = ((unsigned)n + 63u) & ~63u;  // whole waves stay together
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n64; i += gridDim.x * blockDim.x) {
    int32_t c = -1, z = 0;
    unsigned p = 0;
    if (i < (unsigned)n) {
      const int32_t x = xyz[3 * i], y = xyz[3 * i + 1];
      z = xyz[3 * i + 2];
      const int32_t bx = x / bin, by = y / bin;
      int mine = 0;
      if (x < 0 || y < 0 || bx >= w || by >= h)
        mine |= R_XY;
      if (x >= COORD_LIMIT || y >= COORD_LIMIT || z >= COORD_LIMIT || x <= -COORD_LIMIT || y <= -COORD_LIMIT || z <= -COORD_LIMIT)
        mine |= R_COORD;
      bad |= mine;
      if (!mine) {
        p = (unsigned)by * (unsigned)w + (unsigned)bx;
        c = ringimg[p];
        if (c >= nb)  // (a map value out of range: the check of the map has set its flag)
          c = -1;
      }
    }
    // ring_points, one building of the wave at a time: lane 0 adds the number of its lanes once
    unsigned long long todo = __ballot(c >= 0);
    while (todo) {
      const int32_t ck = __shfl(c, __ffsll((long long)todo) - 1);
      const unsigned long long members = __ballot(c == ck);
      if ((threadIdx.x & 63) == 0) {
        if (ck < FIG_CAP)
          atomicAdd(&s_points[ck], (unsigned)__popcll(members));
        else
          atomicAdd(f.w(F_RING_POINTS, ck), (unsigned long long)__popcll(members));
      }
      todo &= ~members;
    }
    if (c >= 0)
      atomicMin(low + p, z);
  }
  for (int o = 32; o > 0; o >>= 1)
    bad |= __shfl_xor(bad, o);
  if ((threadIdx.x & 63) == 0 && bad)
    atomicOr(words + W_RANGE, bad);
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x)
    if (s_points[k])
      atomicAdd(f.w(F_RING_POINTS, k), (unsigned long long)s_points[k]);
}

// ---- 3. pixels ------------------------------------------------------------------------------------------------------------
struct Tables {  // the figures of the buildings below FIG_CAP, in LDS: 24 bytes a building
  unsigned ring[FIG_CAP], ground[FIG_CAP];
  int32_t mn[FIG_CAP], mx[FIG_CAP];
  unsigned long long sum[FIG_CAP];  // (the signed sum in two's complement)
};

__global__ __launch_bounds__(256) void tn_pixels_kernel(const int32_t* __restrict__ ringimg, const int32_t* __restrict__ low,
                                                        long long npix, int32_t nb, unsigned long long* __restrict__ keys,
                                                        Fig f, int* __restrict__ words)
{
  __shared__ Tables T;
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    T.ring[k] = T.ground[k] = 0;
    T.mn[k] = INT32_MAX;
    T.mx[k] = INT32_MIN;
    T.sum[k] = 0;
  }
  __syncthreads();
  const long long n64 = (npix + 63) & ~63ll;  // whole waves stay together
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n64; p += (long long)gridDim.x * blockDim.x) {
    int32_t c = -1, l = INT32_MAX;
    if (p < npix) {
      c = ringimg[p];
      if (c >= nb)
        c = -1;
      if (c >= 0)
        l = low[p];
    }
    const bool has = c >= 0 && l != INT32_MAX;
    wave_append(has, ((unsigned long long)(uint32_t)c << 32) | ((uint32_t)l ^ 0x80000000u), keys, words + W_NKEYS);
    unsigned long long todo = __ballot(c >= 0);
    while (todo) {
      const int32_t ck = __shfl(c, __ffsll((long long)todo) - 1);
      const bool mine = c == ck;
      const unsigned long long members = __ballot(mine), grounded = __ballot(mine && has);
      int32_t mn = mine && has ? l : INT32_MAX, mx = mine && has ? l : INT32_MIN;
      unsigned long long sum = mine && has ? (unsigned long long)(long long)l : 0ull;
      if (grounded)
        for (int o = 32; o > 0; o >>= 1) {
          mn = min(mn, __shfl_xor(mn, o));
          mx = max(mx, __shfl_xor(mx, o));
          sum += __shfl_xor(sum, o);
        }
      if ((threadIdx.x & 63) == 0) {
        const unsigned nr = (unsigned)__popcll(members), ng = (unsigned)__popcll(grounded);
        if (ck < FIG_CAP) {
          atomicAdd(&T.ring[ck], nr);
          if (ng) {
            atomicAdd(&T.ground[ck], ng);
            atomicMin(&T.mn[ck], mn);
            atomicMax(&T.mx[ck], mx);
            atomicAdd(&T.sum[ck], sum);
          }
        } else {
          atomicAdd(f.w(F_RING_PIXELS, ck), (unsigned long long)nr);
          if (ng) {
            atomicAdd(f.w(F_GROUND_PIXELS, ck), (unsigned long long)ng);
            atomicMin(f.n(G_MIN, ck), mn);
            atomicMax(f.n(G_MAX, ck), mx);
            atomicAdd(f.w(F_SUM, ck), sum);
          }
        }
      }
      todo &= ~members;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x) {
    if (!T.ring[k])
      continue;
    atomicAdd(f.w(F_RING_PIXELS, k), (unsigned long long)T.ring[k]);
    if (T.ground[k]) {
      atomicAdd(f.w(F_GROUND_PIXELS, k), (unsigned long long)T.ground[k]);
      atomicMin(f.n(G_MIN, k), T.mn[k]);
      atomicMax(f.n(G_MAX, k), T.mx[k]);
      atomicAdd(f.w(F_SUM, k), T.sum[k]);
    }
  }
}

// ---- 4. pick --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tn_pick_kernel(const unsigned long long* __restrict__ sorted, long long nk,
                                                      const unsigned long long* __restrict__ off, int32_t nb, int32_t q_num,
                                                      int32_t q_den, int32_t min_ground, int32_t fallback_z, Fig f,
                                                      int* __restrict__ words)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nb)
    return;
  const long long g = (long long)*f.w(F_GROUND_PIXELS, c);
  int32_t ground = fallback_z, status = 1;
  if (g >= min_ground) {
    const long long at = (long long)off[c] + (g - 1) * q_num / q_den;
    if (at < 0 || at >= nk || (sorted[at] >> 32) != (unsigned long long)c) {
      atomicOr(words + W_ERR, E_PICK);
    } else {
      ground = (int32_t)((uint32_t)sorted[at] ^ 0x80000000u);
      status = 0;
    }
  }
  *f.n(G_GROUND, c) = ground;
  *f.n(G_STATUS, c) = status;
}

int bits_of(uint32_t v)
{
  int b = 0;
  while (v) {
    b++;
    v >>= 1;
  }
  return b;
}

int check_args(bs_ctx* ctx, const void* xyz, int64_t n, int32_t bin, const void* map, int32_t width, int32_t height,
               int32_t n_buildings, int32_t ring, int32_t q_num, int32_t q_den, int32_t min_ground, const void* out)
{
  if (!xyz || !map || !out)
    return fail(ctx, BS_ERR_INVALID, "terrain: null pointer");
  if (n < 1 || bin < 1)
    return fail(ctx, BS_ERR_INVALID, "terrain: n < 1 or bin < 1");
  if (width < 1 || height < 1 || (long long)width * height >= (1ll << 31))
    return fail(ctx, BS_ERR_INVALID, "terrain: width or height < 1, or width * height >= 2^31");
  if (n_buildings < 0)
    return fail(ctx, BS_ERR_INVALID, "terrain: n_buildings < 0");
  if (ring < 1 || ring > MAX_RING)
    return fail(ctx, BS_ERR_INVALID, "terrain: ring outside 1 .. 255");
  if (q_den < 1 || q_num < 0 || q_num > q_den)
    return fail(ctx, BS_ERR_INVALID, "terrain: the quantile needs 0 <= q_num <= q_den and q_den >= 1");
  if (min_ground < 1)
    return fail(ctx, BS_ERR_INVALID, "terrain: min_ground < 1");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "terrain: 2^29 points or more");
  return BS_OK;
}

int range_error(bs_ctx* ctx, int bits)
{
  if (bits & R_MAP)
    return fail(ctx, BS_ERR_RANGE, "terrain: a map value >= n_buildings");
  if (bits & R_XY)
    return fail(ctx, BS_ERR_RANGE, "terrain: a point with a negative x or y, or whose pixel lies outside the image");
  return fail(ctx, BS_ERR_RANGE, "terrain: a coordinate at or beyond 2^23");
}

// the stage on device inputs; res is zeroed; the three images may be NULL (the scratch images of the context hold them in
// any case: the host-memory twin copies from there)
int terrain(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, const int32_t* d_map, int32_t width, int32_t height,
            int32_t nb, int32_t ring, int32_t q_num, int32_t q_den, int32_t min_ground, int32_t fallback_z, int32_t* d_owner,
            uint8_t* d_dist, int32_t* d_low, struct bs_terrain& res)
{
  const long long npix = (long long)width * height;
  const size_t np = (size_t)npix, nbs = (size_t)nb, nb1 = std::max<size_t>(nbs, 1);
  res.width = width;
  res.height = height;
  res.n_buildings = nb;
  res.bin = bin;
  res.ring = ring;
  res.q_num = q_num;
  res.q_den = q_den;
  res.min_ground = min_ground;
  res.fallback_z = fallback_z;
  res.fig_cap = FIG_CAP;
  res.grid = GRID;
  res.n_points = n;
  int64_t** const wide[F_WIDE] = {&res.ring_pixels, &res.ground_pixels, &res.ring_points, &res.ground_sum};
  int32_t** const narrow[G_NARROW] = {&res.ground_min, &res.ground_max, &res.ground, &res.status};
  for (auto a : wide)
    if (!alloc(a, nbs))
      return fail(ctx, BS_ERR_NOMEM, "terrain: host allocation");
  for (auto a : narrow)
    if (!alloc(a, nbs))
      return fail(ctx, BS_ERR_NOMEM, "terrain: host allocation");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->tn;
  Events<5> ev;
  for (int i = 0; i < 5; i++)
    BS_HIP(ctx, hipEventCreate(&ev.e[i]));
  const size_t fig_bytes = (8 * (size_t)F_WIDE + 4 * (size_t)G_NARROW) * nb1;
  BS_HIP(ctx, B[TN_MISC].reserve(4 * W_WORDS));
  BS_HIP(ctx, B[TN_OWNER].reserve(4 * np));
  BS_HIP(ctx, B[TN_RING].reserve(4 * np));
  BS_HIP(ctx, B[TN_NEXT].reserve(4 * np));
  BS_HIP(ctx, B[TN_DIST].reserve(np));
  BS_HIP(ctx, B[TN_LOW].reserve(4 * np));
  BS_HIP(ctx, B[TN_LIST_A].reserve(4 * np));
  BS_HIP(ctx, B[TN_LIST_B].reserve(4 * np));
  BS_HIP(ctx, B[TN_KEYS].reserve(8 * np));
  BS_HIP(ctx, B[TN_FIG].reserve(fig_bytes));
  BS_HIP(ctx, B[TN_OFF].reserve(8 * nb1));
  int* d_words = B[TN_MISC].as<int>();
  int32_t* owner = B[TN_OWNER].as<int32_t>();
  int32_t* ringimg = B[TN_RING].as<int32_t>();
  int32_t* next = B[TN_NEXT].as<int32_t>();
  uint8_t* dist = B[TN_DIST].as<uint8_t>();
  int32_t* low = B[TN_LOW].as<int32_t>();
  int32_t* lists[2] = {B[TN_LIST_A].as<int32_t>(), B[TN_LIST_B].as<int32_t>()};
  unsigned long long* keys = B[TN_KEYS].as<unsigned long long>();
  unsigned long long* off = B[TN_OFF].as<unsigned long long>();
  const Fig f{B[TN_FIG].as<unsigned long long>(), reinterpret_cast<int32_t*>(B[TN_FIG].as<unsigned long long>() + F_WIDE * nb1),
              (long long)nb1};
  int h_words[4] = {0, 0, 0, 0};  // W_RANGE, W_ERR, W_ROUNDS, W_NKEYS

  // 1. ring
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_words, 0, 4 * W_WORDS, st));
  tn_init_kernel<<<nblk(npix, 256), 256, 0, st>>>(d_map, width, height, nb, owner, ringimg, next, dist, low, lists[0], d_words);
  const int rgrid = (int)std::max<int64_t>(1, std::min<int64_t>(nblk(npix, 256), RING_GRID));
  if (nb > 0)
    for (int r = 1; r <= ring; r++) {
      int32_t* cur = lists[(r - 1) & 1];
      int32_t* nxt = lists[r & 1];
      tn_push_kernel<<<rgrid, 256, 0, st>>>(owner, width, height, cur, d_words + W_CNT + r - 1, next, nxt, d_words + W_CNT + r);
      tn_commit_kernel<<<rgrid, 256, 0, st>>>(nxt, d_words + W_CNT + r, next, r, owner, ringimg, dist, d_words + W_ROUNDS);
    }
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  // 2. points
  tn_fig_init_kernel<<<nblk(nb1, 256), 256, 0, st>>>(f, nb);
  tn_points_kernel<<<(int)std::max<long long>(1, std::min<long long>(nblk(n, 256), GRID)), 256, 0, st>>>(d_xyz, n, bin, width, height, nb,
                                                                                                      ringimg, low, f, d_words);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  // 3. pixels
  tn_pixels_kernel<<<(int)std::max<long long>(1, std::min<long long>(nblk(npix, 256), PIX_GRID)), 256, 0, st>>>(ringimg, low, npix, nb,
                                                                                                             keys, f, d_words);
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, sizeof h_words, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the range flags and the number of keys, before anything of the caller's is written
  BS_HIP(ctx, hipGetLastError());
  if (h_words[W_RANGE])
    return range_error(ctx, h_words[W_RANGE]);
  const long long nk = h_words[W_NKEYS];
  if (nk < 0 || nk > npix)
    return fail(ctx, BS_ERR_INTERNAL, "terrain: the key count left its range");
  // 4. pick
  const unsigned long long* sorted = keys;
  if (nb > 0) {
    if (nk > 0) {
      const int end_bit = 32 + std::max(bits_of((uint32_t)nb - 1u), 1);
      BS_HIP(ctx, B[TN_SORTED].reserve(8 * (size_t)nk));
      BS_HIP(ctx, cub_run(B[TN_TMP], [&](void* tmp, size_t& bytes) {
        return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys, B[TN_SORTED].as<unsigned long long>(), (int)nk, 0, end_bit, st);
      }));
      sorted = B[TN_SORTED].as<unsigned long long>();
    }
    BS_HIP(ctx, cub_run(B[TN_TMP], [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, f.wide + F_GROUND_PIXELS * (long long)nb1, off, nb, st);
    }));
    tn_pick_kernel<<<nblk(nb, 256), 256, 0, st>>>(sorted, nk, off, nb, q_num, q_den, min_ground, fallback_z, f, d_words);
  }
  std::vector<unsigned char> h_fig(fig_bytes);
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, sizeof h_words, hipMemcpyDeviceToHost, st));
  if (nb > 0)
    BS_HIP(ctx, hipMemcpyAsync(h_fig.data(), B[TN_FIG].p, fig_bytes, hipMemcpyDeviceToHost, st));
  // the caller's images: the ranges are known, and the images do not depend on the pick
  if (d_owner)
    BS_HIP(ctx, hipMemcpyAsync(d_owner, owner, 4 * np, hipMemcpyDeviceToDevice, st));
  if (d_dist)
    BS_HIP(ctx, hipMemcpyAsync(d_dist, dist, np, hipMemcpyDeviceToDevice, st));
  if (d_low)
    BS_HIP(ctx, hipMemcpyAsync(d_low, low, 4 * np, hipMemcpyDeviceToDevice, st));
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  if (h_words[W_ERR])
    return fail(ctx, BS_ERR_INTERNAL, "terrain: a sorted key is not its building's");
  const unsigned long long* hw = reinterpret_cast<const unsigned long long*>(h_fig.data());
  const int32_t* hn = reinterpret_cast<const int32_t*>(hw + F_WIDE * nb1);
  for (size_t c = 0; c < nbs; c++) {
    for (int j = 0; j < F_WIDE; j++)
      (*wide[j])[c] = (int64_t)hw[(size_t)j * nb1 + c];
    for (int j = 0; j < G_NARROW; j++)
      (*narrow[j])[c] = hn[(size_t)j * nb1 + c];
    res.n_ring_pixels += res.ring_pixels[c];
    res.n_ground_pixels += res.ground_pixels[c];
    res.n_ring_points += res.ring_points[c];
    res.n_fallback += res.status[c] != 0;
  }
  res.rounds_used = h_words[W_ROUNDS];
  res.ms_ring = ev.ms(0, 1);
  res.ms_points = ev.ms(1, 2);
  res.ms_pixels = ev.ms(2, 3);
  res.ms_pick = ev.ms(3, 4);
  return BS_OK;
}

using TGuard = FreeUnlessKept<struct bs_terrain, bs_terrain_free>;

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_terrain_free(struct bs_terrain* t)
{
  if (!t)
    return;
  free(t->ring_pixels);
  free(t->ground_pixels);
  free(t->ring_points);
  free(t->ground_sum);
  free(t->ground_min);
  free(t->ground_max);
  free(t->ground);
  free(t->status);
  memset(t, 0, sizeof *t);
}

extern "C" int bs_terrain_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, const int32_t* d_map, int32_t width,
                              int32_t height, int32_t n_buildings, int32_t ring, int32_t q_num, int32_t q_den,
                              int32_t min_ground, int32_t fallback_z, int32_t* d_owner, uint8_t* d_dist, int32_t* d_low,
                              struct bs_terrain* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int rc = check_args(ctx, d_xyz, n, bin, d_map, width, height, n_buildings, ring, q_num, q_den, min_ground, out);
  if (rc != BS_OK)
    return rc;
  struct bs_terrain res;
  memset(&res, 0, sizeof res);
  TGuard guard{&res};
  rc = terrain(ctx, d_xyz, n, bin, d_map, width, height, n_buildings, ring, q_num, q_den, min_ground, fallback_z, d_owner, d_dist,
               d_low, res);
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  *out = res;
  return BS_OK;
}

extern "C" int bs_terrain(bs_ctx* ctx, const int32_t* xyz, int64_t n, int32_t bin, const int32_t* map, int32_t width,
                          int32_t height, int32_t n_buildings, int32_t ring, int32_t q_num, int32_t q_den, int32_t min_ground,
                          int32_t fallback_z, int32_t* owner, uint8_t* dist, int32_t* low, struct bs_terrain* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int rc = check_args(ctx, xyz, n, bin, map, width, height, n_buildings, ring, q_num, q_den, min_ground, out);
  if (rc != BS_OK)
    return rc;
  struct bs_terrain res;
  memset(&res, 0, sizeof res);
  TGuard guard{&res};
  DevBuf* B = ctx->tn;
  const size_t np = (size_t)width * (size_t)height;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(B[TN_IN_XYZ], xyz, 3 * (size_t)n);
  const int32_t* d_map = S.upload(B[TN_IN_MAP], map, np);
  if (!S.ok())
    return S.status();
  rc = terrain(ctx, d_xyz, n, bin, d_map, width, height, n_buildings, ring, q_num, q_den, min_ground, fallback_z, nullptr, nullptr,
               nullptr, res);
  if (rc != BS_OK)
    return rc;
  S.download(owner, B[TN_OWNER].as<int32_t>(), np);
  S.download(dist, B[TN_DIST].as<uint8_t>(), np);
  S.download(low, B[TN_LOW].as<int32_t>(), np);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  *out = res;
  return BS_OK;
}
