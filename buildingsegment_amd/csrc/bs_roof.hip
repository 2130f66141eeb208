// bs_roof.hip -- which plane is the roof over every pixel of a building, and how high it is there (DESIGN.md §4,
// "Roofs"; the definition is written down in include/bs_api.h).
//   1. vote     every counting point emits the 64-bit key pixel * n_planes + (plane - 1), compacted as it is written
//               (most points of a cloud are ground or wall: one slot range per 2048 points), then one radix sort over the bits
//               in use + run lengths give the exact count of every (pixel, plane); one 64-bit atomicMax per run on
//               (count << 32) | ~plane leaves every pixel its winner (largest count, then lowest id).  The seed pass
//               writes roof / support and lists the seeds that touch an unlabelled pixel of their building.
//   2. fill     frontier worklists: a frontier pixel pushes its plane to its unlabelled same-building 4-neighbours with
//               atomicMin on next[]; the first pusher appends the neighbour to the next list (one atomicAdd per wave
//               and direction); a separate commit kernel writes roof from next[] once the round's pushes are done, so
//               a label moves one pixel per round.  Rounds are launched in groups of FILL_GROUP whose kernels leave at
//               once on an empty list; the host reads one count per group.  No pass over the image per round.
//   3. figures  one pass over the points (the wave in one plane: registers; planes <= FIG_CAP: LDS tables flushed once
//               per workgroup and plane; the rest: global atomics) and one over the pixels (per run of equal roof
//               inside a wave)
//   4. heights  one pixel pass: the plane's height at the pixel centre, clamped to the plane's own supporting points
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bs_common.h"
#include "bs_host.h"
#include "bs_roofheight.h"

namespace bs {
namespace {

constexpr int FIG_CAP = 2048;  // planes 1 .. FIG_CAP: point and pixel figures reduced in LDS (40 KB and 48 KB)
constexpr int KEY_ITEMS = 8;   // points per thread of the key pass: one slot range per 2048 points
constexpr int FILL_GROUP = 8;  // fill rounds launched per host round trip (even: the lists alternate)
constexpr int FILL_GRID = 512; // workgroups of a fill kernel (grid-stride over the list)
// scratch of bs_ctx::rf
enum { RF_KEYS, RF_KEYS2, RF_RUNS, RF_TMP, RF_BEST, RF_NEXT, RF_LIST_A, RF_LIST_B, RF_MISC, RF_TAB, RF_FIG, RF_IN_XYZ,
       RF_IN_MAP, RF_IN_PLANE, RF_OUT, RF_COUNT };
static_assert(RF_COUNT <= (int)(sizeof(bs_ctx::rf) / sizeof(DevBuf)), "bs_ctx::rf is too short");

struct Tables {  // per plane, device: entry p - 1 is plane p
  const int32_t* home;
  const double* normal;
  const int32_t* center;
};

// the plane (0-based) a point counts for and its pixel; -1: it does not count; -2: its pixel lies outside the image
__device__ inline int32_t counting(const int32_t* __restrict__ xyz, int64_t i, int bin, double ground_th, GroundRule rule,
                                   const int32_t* __restrict__ map, int w, int h, const int32_t* __restrict__ plane,
                                   int32_t npl, const int32_t* __restrict__ home, int64_t* pix, int32_t* zout)
{
  const int32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  const int32_t px = x / bin, py = y / bin;  // base pixel, as bs_assign_buildings
  if (x < 0 || y < 0 || px >= w || py >= h)
    return -2;
  *pix = (int64_t)py * w + px;
  *zout = z;
  const int32_t p = plane[i];
  if (p < 1 || p > npl || rule.below(x, y, z, ground_th))
    return -1;
  const int32_t b = map[*pix];
  return (b >= 0 && home[p - 1] == b) ? p - 1 : -1;
}

// The keys of the counting points, compacted (most points of a cloud are ground or wall; the order does not matter:
// the keys are sorted next): a workgroup takes KEY_ITEMS * 256 consecutive points and one slot range for all of them.
__global__ __launch_bounds__(256) void keys_kernel(const int32_t* __restrict__ xyz, int64_t n, int bin, double ground_th, GroundRule rule,
                                                   const int32_t* __restrict__ map, int w, int h,
                                                   const int32_t* __restrict__ plane, int32_t npl,
                                                   const int32_t* __restrict__ home, uint64_t* __restrict__ keys,
                                                   int32_t* __restrict__ n_keys, int* __restrict__ bad)
{
  __shared__ int s_wave[4];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t base = blockIdx.x * (int64_t)(256 * KEY_ITEMS);
  uint64_t key[KEY_ITEMS];
  unsigned long long mask[KEY_ITEMS];
  int wtot = 0;
#pragma unroll
  for (int j = 0; j < KEY_ITEMS; j++) {
    const int64_t i = base + j * 256 + threadIdx.x;
    int32_t s = -1, z;
    int64_t pix = 0;
    if (i < n) {
      s = counting(xyz, i, bin, ground_th, rule, map, w, h, plane, npl, home, &pix, &z);
      if (s == -2)
        atomicOr(bad, 1);
    }
    key[j] = s < 0 ? 0 : (uint64_t)pix * (uint64_t)npl + (uint64_t)s;
    mask[j] = __ballot(s >= 0);
    wtot += (int)__popcll(mask[j]);
  }
  if (lane == 0)
    s_wave[wv] = wtot;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = tot ? atomicAdd(n_keys, tot) : 0;
  }
  __syncthreads();
  int off = s_base;
  for (int v = 0; v < wv; v++)
    off += s_wave[v];
#pragma unroll
  for (int j = 0; j < KEY_ITEMS; j++) {
    if ((mask[j] >> lane) & 1)
      keys[off + __popcll(mask[j] & ((1ull << lane) - 1))] = key[j];
    off += (int)__popcll(mask[j]);
  }
}

// best[pixel] = max over its runs of (count << 32) | ~plane: the largest count, then the lowest plane id
__global__ __launch_bounds__(256) void runs_kernel(const uint64_t* __restrict__ key, const int32_t* __restrict__ len,
                                                   const int32_t* __restrict__ n_runs, uint64_t none, int32_t npl,
                                                   unsigned long long* __restrict__ best)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= *n_runs || key[r] >= none)
    return;
  const uint64_t pix = key[r] / (uint64_t)npl;
  const uint32_t p = (uint32_t)(key[r] - pix * (uint64_t)npl) + 1u;
  atomicMax(best + pix, ((unsigned long long)(uint32_t)len[r] << 32) | (0xFFFFFFFFu - p));
}

__device__ inline bool seeded(unsigned long long best, int32_t min_votes) { return (best >> 32) >= (unsigned)min_votes; }

// append v of the lanes with `take` to list[*count ...]: one atomicAdd per wave (every lane of the wave calls this)
__device__ inline void wave_append(bool take, int32_t v, int32_t* __restrict__ list, int32_t* __restrict__ count)
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

// roof / support of the vote, next[] = "no push yet", and the first frontier: the seeds with an unseeded 4-neighbour
// in their own building
__global__ __launch_bounds__(256) void seed_kernel(const int32_t* __restrict__ map,
                                                   const unsigned long long* __restrict__ best, int w, int h,
                                                   int32_t min_votes, int32_t* __restrict__ roof,
                                                   int32_t* __restrict__ support, int32_t* __restrict__ next,
                                                   int32_t* __restrict__ list, int32_t* __restrict__ count)
{
  const int64_t npix = (int64_t)w * h, i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool front = false;
  if (i < npix) {
    const int32_t b = map[i];
    const unsigned long long v = best[i];
    const bool sd = b >= 0 && seeded(v, min_votes);
    roof[i] = b < 0 ? -1 : (sd ? (int32_t)(0xFFFFFFFFu - (uint32_t)v) : 0);
    if (support)
      support[i] = sd ? (int32_t)(v >> 32) : 0;
    next[i] = INT32_MAX;
    if (sd) {
      const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
      front = (x > 0 && map[i - 1] == b && !seeded(best[i - 1], min_votes)) ||
              (x < w - 1 && map[i + 1] == b && !seeded(best[i + 1], min_votes)) ||
              (y > 0 && map[i - w] == b && !seeded(best[i - w], min_votes)) ||
              (y < h - 1 && map[i + w] == b && !seeded(best[i + w], min_votes));
    }
  }
  block_append(front, (int32_t)i, list, count);
}

// One round, first half: the pixels of `cur` (labelled in the round before) push their plane to their unlabelled
// 4-neighbours of the same building.  roof is only read here: whatever this round labels is written by the commit.
__global__ __launch_bounds__(256) void fill_push_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ roof,
                                                        int w, int h, const int32_t* __restrict__ cur,
                                                        const int32_t* __restrict__ n_cur, int32_t* __restrict__ next,
                                                        int32_t* __restrict__ out, int32_t* __restrict__ n_out)
{
  const int64_t cnt = *n_cur;
  if (cnt == 0)
    return;
  const int64_t cnt64 = (cnt + 63) & ~(int64_t)63, stride = (int64_t)gridDim.x * blockDim.x;  // whole waves stay together
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < cnt64; t += stride) {
    int32_t pix = -1, p = 0, b = 0;
    int x = 0, y = 0;
    if (t < cnt) {
      pix = cur[t];
      p = roof[pix];
      b = map[pix];
      y = pix / w;
      x = pix - y * w;
    }
    for (int d = 0; d < 4; d++) {
      const int nx = x + (d == 0) - (d == 1), ny = y + (d == 2) - (d == 3);
      bool won = false;
      int32_t q = 0;
      if (pix >= 0 && nx >= 0 && nx < w && ny >= 0 && ny < h) {
        q = ny * w + nx;
        if (map[q] == b && roof[q] == 0)
          won = atomicMin(next + q, p) == INT32_MAX;  // the first pusher lists the pixel
      }
      wave_append(won, q, out, n_out);
    }
  }
}

// One round, second half: the pixels the round reached take the smallest plane that was pushed to them.
__global__ __launch_bounds__(256) void fill_commit_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ n_list,
                                                          const int32_t* __restrict__ next, int32_t* __restrict__ roof,
                                                          int32_t* __restrict__ rounds)
{
  const int64_t cnt = *n_list;
  if (cnt == 0)
    return;
  const int64_t first = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t t = first; t < cnt; t += (int64_t)gridDim.x * blockDim.x) {
    const int32_t q = list[t];
    roof[q] = next[q];
  }
  if (first == 0)
    *rounds += 1;  // (one writer: the kernels of a stream run one after the other)
}

// ---- figures -----------------------------------------------------------------------------------------------------
struct Fig {  // per plane, device
  unsigned long long* pixels;
  unsigned long long* seed_pixels;
  unsigned long long* n_support;
  unsigned long long* z_sum;
  int32_t* bbox;
  int32_t* z_min;
  int32_t* z_max;
  unsigned long long* totals;  // seeded, roofed, unroofed pixels
};

__global__ __launch_bounds__(256) void fig_init_kernel(Fig f, int32_t npl)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < 3)
    f.totals[c] = 0;
  if (c >= npl)
    return;
  f.pixels[c] = f.seed_pixels[c] = f.n_support[c] = f.z_sum[c] = 0;
  f.bbox[4 * c] = f.bbox[4 * c + 1] = f.z_min[c] = INT32_MAX;
  f.bbox[4 * c + 2] = f.bbox[4 * c + 3] = f.z_max[c] = INT32_MIN;
}

__device__ inline void ptfig_global(const Fig& f, int32_t s, unsigned cnt, int32_t mn, int32_t mx, unsigned long long zs)
{
  atomicAdd(f.n_support + s, (unsigned long long)cnt);
  atomicMin(f.z_min + s, mn);
  atomicMax(f.z_max + s, mx);
  atomicAdd(f.z_sum + s, zs);
}

// A supporting point is a counting point whose plane is the final roof of its pixel.
__global__ __launch_bounds__(256) void ptfig_kernel(const int32_t* __restrict__ xyz, int64_t n, int bin, double ground_th, GroundRule rule,
                                                    const int32_t* __restrict__ map, int w, int h,
                                                    const int32_t* __restrict__ plane, int32_t npl,
                                                    const int32_t* __restrict__ home, const int32_t* __restrict__ roof,
                                                    Fig f)
{
  __shared__ unsigned s_cnt[FIG_CAP];
  __shared__ int s_mn[FIG_CAP], s_mx[FIG_CAP];
  __shared__ unsigned long long s_sum[FIG_CAP];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    s_cnt[k] = 0;
    s_mn[k] = INT32_MAX;
    s_mx[k] = INT32_MIN;
    s_sum[k] = 0;
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, n64 = (n + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n64; i += stride) {
    int32_t s = -1, z = 0;
    if (i < n) {
      int64_t pix = 0;
      s = counting(xyz, i, bin, ground_th, rule, map, w, h, plane, npl, home, &pix, &z);
      if (s >= 0 && roof[pix] != s + 1)
        s = -1;
      if (s < 0)
        s = -1;
    }
    const int32_t s0 = __shfl(s, 0);
    if (__all(s == s0)) {  // the whole wave supports one plane (clouds in spatial order): reduce in registers
      if (s0 < 0)
        continue;
      int32_t mn = z, mx = z;
      unsigned long long zs = (unsigned long long)(long long)z;
      for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, __shfl_xor(mn, o));
        mx = max(mx, __shfl_xor(mx, o));
        zs += __shfl_xor(zs, o);
      }
      if ((threadIdx.x & 63) == 0) {
        if (s0 < FIG_CAP) {
          atomicAdd(s_cnt + s0, 64u);
          atomicMin(s_mn + s0, mn);
          atomicMax(s_mx + s0, mx);
          atomicAdd(s_sum + s0, zs);
        } else {
          ptfig_global(f, s0, 64u, mn, mx, zs);
        }
      }
    } else if (s >= 0) {
      if (s < FIG_CAP) {
        atomicAdd(s_cnt + s, 1u);
        atomicMin(s_mn + s, z);
        atomicMax(s_mx + s, z);
        atomicAdd(s_sum + s, (unsigned long long)(long long)z);
      } else {
        ptfig_global(f, s, 1u, z, z, (unsigned long long)(long long)z);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < npl; k += blockDim.x)
    if (s_cnt[k])
      ptfig_global(f, k, s_cnt[k], s_mn[k], s_mx[k], s_sum[k]);
}

__device__ inline void pixfig_global(const Fig& f, int32_t s, unsigned pix, unsigned nseed, int x0, int y0, int x1, int y1)
{
  atomicAdd(f.pixels + s, (unsigned long long)pix);
  if (nseed)
    atomicAdd(f.seed_pixels + s, (unsigned long long)nseed);
  atomicMin(f.bbox + 4 * s, x0);
  atomicMin(f.bbox + 4 * s + 1, y0);
  atomicMax(f.bbox + 4 * s + 2, x1);
  atomicMax(f.bbox + 4 * s + 3, y1);
}

// The pixel figures leave a wave once per run of equal roof inside its 64 consecutive pixels of one row (map_kernel's
// scheme in bs_building.hip); the three totals once per workgroup.
__global__ __launch_bounds__(256) void pixfig_kernel(const int32_t* __restrict__ roof,
                                                     const unsigned long long* __restrict__ best, int w, int h,
                                                     int32_t min_votes, int32_t npl, Fig f)
{
  __shared__ unsigned s_pix[FIG_CAP], s_seed[FIG_CAP];
  __shared__ int s_x0[FIG_CAP], s_y0[FIG_CAP], s_x1[FIG_CAP], s_y1[FIG_CAP];
  __shared__ unsigned long long s_tot[3];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    s_pix[k] = s_seed[k] = 0;
    s_x0[k] = s_y0[k] = INT32_MAX;
    s_x1[k] = s_y1[k] = INT32_MIN;
  }
  if (threadIdx.x < 3)
    s_tot[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t npix = (int64_t)w * h, npix64 = (npix + 63) & ~(int64_t)63;
  for (int64_t base = blockIdx.x * (int64_t)blockDim.x; base < npix64; base += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = base + threadIdx.x;
    if (i >= npix64)
      continue;  // (whole waves: npix64 is a multiple of 64)
    int32_t r = -1;
    int x = 0, y = 0;
    bool sd = false;
    if (i < npix) {
      y = (int)(i / w);
      x = (int)(i - (int64_t)y * w);
      r = roof[i];
      if (r > npl)
        r = -1;  // (stay in bounds)
      sd = r > 0 && seeded(best[i], min_votes);
    }
    const int32_t prev = __shfl_up(r, 1);
    const bool head = lane == 0 || prev != r || x == 0;
    const unsigned long long heads = __ballot(head), sdm = __ballot(sd), roofed = __ballot(r > 0), un = __ballot(r == 0);
    if (lane == 0) {
      if (sdm)
        atomicAdd(s_tot, (unsigned long long)__popcll(sdm));
      if (roofed)
        atomicAdd(s_tot + 1, (unsigned long long)__popcll(roofed));
      if (un)
        atomicAdd(s_tot + 2, (unsigned long long)__popcll(un));
    }
    if (head && r > 0) {
      const unsigned long long above = lane == 63 ? 0 : heads & (~0ull << (lane + 1));
      const int end = above ? __ffsll((long long)above) - 1 : 64;  // one past the run's last lane
      const int len = end - lane;
      const unsigned long long run = (len == 64 ? ~0ull : ((1ull << len) - 1)) << lane;
      const unsigned nseed = (unsigned)__popcll(sdm & run);
      const int32_t s = r - 1;
      if (s < FIG_CAP) {
        atomicAdd(s_pix + s, (unsigned)len);
        if (nseed)
          atomicAdd(s_seed + s, nseed);
        atomicMin(s_x0 + s, x);
        atomicMin(s_y0 + s, y);
        atomicMax(s_x1 + s, x + len - 1);
        atomicMax(s_y1 + s, y);
      } else {
        pixfig_global(f, s, (unsigned)len, nseed, x, y, x + len - 1, y);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < npl; k += blockDim.x)
    if (s_pix[k])
      pixfig_global(f, k, s_pix[k], s_seed[k], s_x0[k], s_y0[k], s_x1[k], s_y1[k]);
  if (threadIdx.x < 3 && s_tot[threadIdx.x])
    atomicAdd(f.totals + threadIdx.x, s_tot[threadIdx.x]);
}

__global__ __launch_bounds__(256) void height_kernel(const int32_t* __restrict__ roof, int w, int h, int bin, int32_t npl,
                                                     Tables t, const int32_t* __restrict__ z_min,
                                                     const int32_t* __restrict__ z_max, int32_t* __restrict__ height)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= (int64_t)w * h)
    return;
  const int32_t r = roof[i];
  int32_t v = INT32_MIN;
  if (r > 0 && r <= npl) {
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    const int32_t s = r - 1;
    v = (int32_t)roof_height(t.normal + 3 * s, t.center + 3 * s, z_min[s], z_max[s], (int64_t)x * bin + bin / 2,
                             (int64_t)y * bin + bin / 2);
  }
  height[i] = v;
}

bool alloc_roofs(struct bs_roofs* r, int32_t npl)
{
  const size_t m = (size_t)std::max(npl, 1);
  r->pixels = (int64_t*)calloc(m, 8);
  r->seed_pixels = (int64_t*)calloc(m, 8);
  r->bbox = (int32_t*)calloc(4 * m, 4);
  r->n_support = (int64_t*)calloc(m, 8);
  r->z_min = (int32_t*)calloc(m, 4);
  r->z_max = (int32_t*)calloc(m, 4);
  r->z_sum = (int64_t*)calloc(m, 8);
  return r->pixels && r->seed_pixels && r->bbox && r->n_support && r->z_min && r->z_max && r->z_sum;
}

bool bad_image(int32_t w, int32_t h) { return w < 1 || h < 1 || (int64_t)w * h >= (1ll << 31); }

const char* const ROOFS_INVALID =
    "roofs: null pointer, n < 1, bin < 1, width or height < 1, n_planes < 0 or min_votes < 1";

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_roofs_free(struct bs_roofs* r)
{
  if (!r)
    return;
  free(r->pixels);
  free(r->seed_pixels);
  free(r->bbox);
  free(r->n_support);
  free(r->z_min);
  free(r->z_max);
  free(r->z_sum);
  memset(r, 0, sizeof *r);
}

extern "C" int bs_roof_homes(const double* normal, const int32_t* plane_building, const int64_t* votes_in,
                             const int64_t* votes_total, int32_t n_planes, double min_normal_z, int32_t* home_out)
{
  if (n_planes < 0 || (n_planes > 0 && (!normal || !plane_building || !votes_in || !votes_total || !home_out)))
    return BS_ERR_INVALID;
  for (int32_t p = 0; p < n_planes; p++) {
    const bool ok = normal[3 * p + 2] >= min_normal_z && plane_building[p] >= 0 && 2 * votes_in[p] > votes_total[p];
    home_out[p] = ok ? plane_building[p] : -1;
  }
  return BS_OK;
}

extern "C" int bs_roofs_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, double ground_th,
                            const int32_t* d_map, int32_t width, int32_t height, const int32_t* d_plane_idx,
                            int32_t n_planes, const int32_t* home, const double* normal, const int32_t* center,
                            int32_t min_votes, int32_t* d_roof, int32_t* d_support, int32_t* d_height, struct bs_roofs* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (out)
    memset(out, 0, sizeof *out);
  if (!d_xyz || !d_map || !d_plane_idx || !d_roof || !out || n < 1 || bin < 1 || bad_image(width, height) ||
      n_planes < 0 || min_votes < 1 || (n_planes > 0 && (!home || !normal || !center)))
    return fail(ctx, BS_ERR_INVALID, ROOFS_INVALID);
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "roofs: 2^29 points or more");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int w = width, h = height;
  const int32_t npl = n_planes;
  const int64_t npix = (int64_t)w * h;
  const size_t m = (size_t)std::max(npl, 1);
  DevBuf* B = ctx->rf;
  Events<5> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));

  const uint64_t none = (uint64_t)npix * (uint64_t)npl;  // one past the largest key
  int bits = 1;
  while (bits < 64 && (1ull << bits) <= none)
    bits++;
  BS_HIP(ctx, B[RF_KEYS].reserve(8 * (size_t)n));
  BS_HIP(ctx, B[RF_KEYS2].reserve(8 * (size_t)n));
  BS_HIP(ctx, B[RF_RUNS].reserve(12 * (size_t)n));
  BS_HIP(ctx, B[RF_BEST].reserve(8 * (size_t)npix));
  BS_HIP(ctx, B[RF_NEXT].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[RF_LIST_A].reserve(4 * (size_t)npix + 256));
  BS_HIP(ctx, B[RF_LIST_B].reserve(4 * (size_t)npix + 256));
  BS_HIP(ctx, B[RF_MISC].reserve(256));
  BS_HIP(ctx, B[RF_TAB].reserve(40 * m));
  BS_HIP(ctx, B[RF_FIG].reserve(56 * m + 64));
  uint64_t* keys = B[RF_KEYS].as<uint64_t>();
  uint64_t* sorted = B[RF_KEYS2].as<uint64_t>();
  uint64_t* run_key = B[RF_RUNS].as<uint64_t>();
  int32_t* run_len = reinterpret_cast<int32_t*>(run_key + n);
  unsigned long long* best = B[RF_BEST].as<unsigned long long>();
  int32_t* next = B[RF_NEXT].as<int32_t>();
  int32_t* lists[2] = {B[RF_LIST_A].as<int32_t>(), B[RF_LIST_B].as<int32_t>()};
  // [0] bad pixel, [1] runs of the sort, [2] fill rounds, [3] counting points, [4 ..] the list counts
  int* d_bad = B[RF_MISC].as<int>();
  int32_t* d_nruns = d_bad + 1;
  int32_t* d_rounds = d_bad + 2;
  int32_t* d_nkeys = d_bad + 3;
  int32_t* d_cnt = d_bad + 4;          // [FILL_GROUP + 1]: round k of a group reads d_cnt[k] and fills d_cnt[k + 1]
  // the sort and the runs of the votes: sized for every point here, run over the nk points that count
  auto sort = [=](int count) {
    return [=](void* tmp, size_t& bytes) { return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, keys, sorted, count, 0, bits, st); };
  };
  auto runs = [=](int count) {
    return [=](void* tmp, size_t& bytes) {
      return hipcub::DeviceRunLengthEncode::Encode(tmp, bytes, sorted, run_key, run_len, d_nruns, count, st);
    };
  };
  BS_HIP(ctx, npl > 0 ? cub_room(B[RF_TMP], sort((int)n), runs((int)n)) : cub_room(B[RF_TMP]));  // (no plane: neither runs)
  double* tab_normal = B[RF_TAB].as<double>();
  int32_t* tab_center = reinterpret_cast<int32_t*>(tab_normal + 3 * m);
  int32_t* tab_home = tab_center + 3 * m;
  const Tables tab{tab_home, tab_normal, tab_center};
  Fig f;
  f.pixels = B[RF_FIG].as<unsigned long long>();
  f.seed_pixels = f.pixels + m;
  f.n_support = f.seed_pixels + m;
  f.z_sum = f.n_support + m;
  f.totals = f.z_sum + m;
  f.bbox = reinterpret_cast<int32_t*>(f.totals + 4);
  f.z_min = f.bbox + 4 * m;
  f.z_max = f.z_min + m;
  if (npl > 0) {
    BS_HIP(ctx, hipMemcpyAsync(tab_normal, normal, 24 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_center, center, 12 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_home, home, 4 * (size_t)npl, hipMemcpyHostToDevice, st));
  }

  // ---- vote ----
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_bad, 0, 4 * (4 + FILL_GROUP + 1), st));
  BS_HIP(ctx, hipMemsetAsync(best, 0, 8 * (size_t)npix, st));
  keys_kernel<<<nblk(n, 256 * KEY_ITEMS), 256, 0, st>>>(d_xyz, n, bin, ground_th, ground_rule(ctx), d_map, w, h, d_plane_idx, npl, tab_home,
                                                        keys, d_nkeys, d_bad);
  int h_flags[4] = {0, 0, 0, 0};  // (before anything is written to the caller's arrays)
  BS_HIP(ctx, hipMemcpyAsync(h_flags, d_bad, 16, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_flags[0])
    return fail(ctx, BS_ERR_RANGE, "roofs: a point's pixel lies outside the image (cloud not shifted, or another bin?)");
  const int nk = h_flags[3];
  if (npl > 0 && nk > 0) {
    BS_HIP(ctx, cub_run(B[RF_TMP], sort(nk)));
    BS_HIP(ctx, cub_run(B[RF_TMP], runs(nk)));
    runs_kernel<<<nblk(nk, 256), 256, 0, st>>>(run_key, run_len, d_nruns, none, npl, best);
  }
  seed_kernel<<<nblk(npix, 256), 256, 0, st>>>(d_map, best, w, h, min_votes, d_roof, d_support, next, lists[0], d_cnt);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));

  // ---- fill ----
  const int fgrid = (int)std::min<int64_t>(nblk(npix, 256), FILL_GRID);
  static_assert(FILL_GROUP % 2 == 0, "the current list must be lists[0] again after a group");
  for (;;) {
    for (int k = 0; k < FILL_GROUP; k++) {
      int32_t* cur = lists[k & 1];
      int32_t* nxt = lists[(k + 1) & 1];
      fill_push_kernel<<<fgrid, 256, 0, st>>>(d_map, d_roof, w, h, cur, d_cnt + k, next, nxt, d_cnt + k + 1);
      fill_commit_kernel<<<fgrid, 256, 0, st>>>(nxt, d_cnt + k + 1, next, d_roof, d_rounds);
    }
    int32_t h_last = 0;
    BS_HIP(ctx, hipMemcpyAsync(&h_last, d_cnt + FILL_GROUP, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(d_cnt, d_cnt + FILL_GROUP, 4, hipMemcpyDeviceToDevice, st));
    BS_HIP(ctx, hipMemsetAsync(d_cnt + 1, 0, 4 * FILL_GROUP, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    if (h_last == 0)
      break;
  }
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));

  // ---- figures ----
  fig_init_kernel<<<nblk(std::max<int32_t>(npl, 3), 256), 256, 0, st>>>(f, npl);
  ptfig_kernel<<<(int)std::min<int64_t>(nblk(n, 256), 2048), 256, 0, st>>>(d_xyz, n, bin, ground_th, ground_rule(ctx), d_map, w, h,
                                                                          d_plane_idx, npl, tab_home, d_roof, f);
  pixfig_kernel<<<(int)std::min<int64_t>(nblk(npix, 256), 4096), 256, 0, st>>>(d_roof, best, w, h, min_votes, npl, f);
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));

  // ---- heights ----
  if (d_height)
    height_kernel<<<nblk(npix, 256), 256, 0, st>>>(d_roof, w, h, bin, npl, tab, f.z_min, f.z_max, d_height);
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));

  if (!alloc_roofs(out, npl)) {
    bs_roofs_free(out);
    return fail(ctx, BS_ERR_NOMEM, "roofs: host allocation");
  }
  unsigned long long tot[3] = {0, 0, 0};
  int32_t h_rounds = 0;
  BS_HIP(ctx, hipMemcpyAsync(tot, f.totals, 24, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&h_rounds, d_rounds, 4, hipMemcpyDeviceToHost, st));
  if (npl > 0) {
    BS_HIP(ctx, hipMemcpyAsync(out->pixels, f.pixels, 8 * (size_t)npl, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->seed_pixels, f.seed_pixels, 8 * (size_t)npl, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->n_support, f.n_support, 8 * (size_t)npl, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->z_sum, f.z_sum, 8 * (size_t)npl, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->bbox, f.bbox, 16 * (size_t)npl, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->z_min, f.z_min, 4 * (size_t)npl, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(out->z_max, f.z_max, 4 * (size_t)npl, hipMemcpyDeviceToHost, st));
  }
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  out->n_planes = npl;
  out->width = w;
  out->height = h;
  out->fill_rounds = h_rounds;
  out->seeded_pixels = (int64_t)tot[0];
  out->filled_pixels = (int64_t)(tot[1] - tot[0]);
  out->unroofed_pixels = (int64_t)tot[2];
  out->ms_vote = ev.ms(0, 1);
  out->ms_fill = ev.ms(1, 2);
  out->ms_figures = ev.ms(2, 3);
  out->ms_height = d_height ? ev.ms(3, 4) : 0.0;
  return BS_OK;
}

extern "C" int bs_roofs(bs_ctx* ctx, const int32_t* xyz, int64_t n, int32_t bin, double ground_th, const int32_t* map,
                        int32_t width, int32_t height, const int32_t* plane_idx, int32_t n_planes, const int32_t* home,
                        const double* normal, const int32_t* center, int32_t min_votes, int32_t* roof, int32_t* support,
                        int32_t* height_out, struct bs_roofs* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (out)
    memset(out, 0, sizeof *out);
  if (!xyz || !map || !plane_idx || !roof || !out || n < 1 || bin < 1 || bad_image(width, height) || n_planes < 0 ||
      min_votes < 1)
    return fail(ctx, BS_ERR_INVALID, ROOFS_INVALID);
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "roofs: 2^29 points or more");
  const size_t npix = (size_t)width * height;
  DevBuf* B = ctx->rf;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(B[RF_IN_XYZ], xyz, 3 * (size_t)n);
  const int32_t* d_map = S.upload(B[RF_IN_MAP], map, npix);
  const int32_t* d_plane = S.upload(B[RF_IN_PLANE], plane_idx, (size_t)n);
  int32_t* d_roof = S.room<int32_t>(B[RF_OUT], 3 * npix);  // roof | support | height
  if (!S.ok())
    return S.status();
  int32_t* d_support = support ? d_roof + npix : nullptr;
  int32_t* d_height = height_out ? d_roof + 2 * npix : nullptr;
  int rc = bs_roofs_dev(ctx, d_xyz, n, bin, ground_th, d_map, width, height, d_plane, n_planes, home, normal, center, min_votes,
                        d_roof, d_support, d_height, out);
  if (rc != BS_OK)
    return rc;
  FreeUnlessKept<struct bs_roofs, bs_roofs_free> guard{out};
  S.download(roof, d_roof, npix);
  S.download(support, d_support, npix);
  S.download(height_out, d_height, npix);
  rc = S.finish();
  guard.keep = rc == BS_OK;
  return rc;
}

// The format is written down in include/bs_api.h.
extern "C" int bs_roofs_write_obj(const int32_t* roof, const int32_t* map, int32_t width, int32_t height, const struct bs_roofs* r,
                                  const double* normal, const int32_t* center, int32_t bin, const int32_t* origin,
                                  const char* path)
{
  if (!roof || !map || !r || !path || bin < 1 || width < 1 || height < 1 || r->n_planes < 0 ||
      (r->n_planes > 0 && (!normal || !center || !r->pixels || !r->z_min || !r->z_max)))
    return BS_ERR_INVALID;
  const int64_t npix = (int64_t)width * height;
  for (int64_t i = 0; i < npix; i++)
    if (roof[i] > r->n_planes)
      return BS_ERR_INVALID;
  // a run starts where the pixel has a roof in a building and its left neighbour differs in roof or building
  auto in_run = [&](int64_t i) { return map[i] >= 0 && roof[i] >= 1; };
  auto starts = [&](int64_t i, int32_t x) {
    return in_run(i) && (x == 0 || !in_run(i - 1) || roof[i - 1] != roof[i] || map[i - 1] != map[i]);
  };
  int64_t runs = 0;
  for (int32_t y = 0; y < height; y++)
    for (int32_t x = 0; x < width; x++)
      runs += starts((int64_t)y * width + x, x);
  int32_t used = 0;
  for (int32_t p = 0; p < r->n_planes; p++)
    used += r->pixels[p] > 0;
  FILE* f = fopen(path, "w");
  if (!f)
    return BS_ERR_INVALID;
  const int64_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  fprintf(f, "# roof runs: %lld over %d planes\n", (long long)runs, (int)used);
  for (int32_t y = 0; y < height; y++)
    for (int32_t x = 0; x < width; x++) {
      const int64_t i = (int64_t)y * width + x;
      if (!starts(i, x))
        continue;
      int32_t x1 = x;
      while (x1 + 1 < width && !starts(i + (x1 + 1 - x), x1 + 1) && in_run(i + (x1 + 1 - x)))
        x1++;
      const int32_t s = roof[i] - 1;
      const int64_t X[2] = {(int64_t)x * bin, ((int64_t)x1 + 1) * bin}, Y[2] = {(int64_t)y * bin, ((int64_t)y + 1) * bin};
      const int cx[4] = {0, 1, 1, 0}, cy[4] = {0, 0, 1, 1};
      for (int k = 0; k < 4; k++) {
        const int64_t H = roof_height(normal + 3 * s, center + 3 * s, r->z_min[s], r->z_max[s], X[cx[k]], Y[cy[k]]);
        fprintf(f, "v %lld %lld %lld\n", (long long)(X[cx[k]] + o[0]), (long long)(Y[cy[k]] + o[1]), (long long)(H + o[2]));
      }
    }
  for (int64_t q = 0; q < runs; q++)
    fprintf(f, "f %lld %lld %lld %lld\n", (long long)(4 * q + 1), (long long)(4 * q + 2), (long long)(4 * q + 3),
            (long long)(4 * q + 4));
  const bool ok = !ferror(f);
  return (fclose(f) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}
