// bs_evidence.hip -- roof evidence: per pixel, the share of the above-ground points that lie on a plane of good quality, over a
// square window (DESIGN.md "Roof evidence"; the definition is written down in include/bs_api.h under "roof evidence"), and
// bs_plane_quality, the host rule that says which planes are good.
//   counts   one grid-stride pass over the points, BS_GROUND_GRID workgroups: the range check, the ground rule of the context,
//            one byte gathered from the plane table, and ONE 64-bit atomicAdd per counting point into a packed image
//            (planar << 32) | above (n < 2^29: no carry).  A point below ground issues nothing.  Where at least AGG_MIN
//            lanes of a wave share their pixel with the next lane (a cloud in scan or cell order), the wave adds once per
//            distinct pixel instead (ballots over equal pixels); a shuffled cloud never takes that path (DESIGN.md has both
//            measured).
//   window   one kernel, a workgroup per 32 x 32 pixels: the packed tile with an apron of r on every side into LDS (two
//            int32 planes), a running window sum along x (a thread per row and plane, in place: lw steps whatever r is),
//            the same along y (a thread per column and plane), then keep, the optional images and the figures.  The figures
//            are reduced per wave in registers, per workgroup in LDS, and added once per workgroup.
// The counts go to scratch of the context; the host waits once for the range word before the window kernel writes anything of
// the caller's, and once for the figures.  Every index is checked before it is used as an address.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>

#include "bs_common.h"
#include "bs_host.h"

namespace bs {
namespace {

// scratch of bs_ctx::evd
enum { EV_MISC, EV_PACKED, EV_OK, EV_IN_XYZ, EV_IN_PLANE, EV_KEEP, EV_ABOVE, EV_PLANAR, EV_WIN_ABOVE, EV_WIN_PLANAR, EV_COUNT };
static_assert(EV_COUNT <= (int)(sizeof(bs_ctx::evd) / sizeof(DevBuf)), "bs_ctx::evd is too short");

constexpr int GRID = BS_GROUND_GRID;    // workgroups of the pass over the points
constexpr int TILE = BS_EVIDENCE_TILE;  // outputs of a workgroup of the window kernel: TILE x TILE
constexpr int WIN_GRID = BS_EVIDENCE_GRID;
constexpr int RMAX = BS_EVIDENCE_RMAX;
constexpr int LW = TILE + 2 * RMAX;  // the widest LDS tile
constexpr int AGG_MIN = 8;           // lanes of a wave that repeat their neighbour's pixel before the wave aggregates
constexpr int LS = LW + 1;           // its row stride: odd, so threads that walk neighbouring rows hit different banks
static_assert(TILE == 32 && 2 * TILE <= 256 && 2 * LW <= 256, "the window kernel runs a thread per row / column and plane");

// the 64-bit words of EV_MISC
enum { M_RANGE, M_COUNTED, M_PLANAR, M_PIXELS, M_KEPT, M_REJECTED, M_THIN, M_MAX, M_WORDS };

// ---- 1. counts ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ev_count_kernel(const int32_t* __restrict__ xyz, long long n,
                                                       const int32_t* __restrict__ plane_idx, int32_t n_planes,
                                                       const uint8_t* __restrict__ ok, int32_t bin, int32_t w, int32_t h,
                                                       double ground_th, GroundRule rule,
                                                       unsigned long long* __restrict__ packed,
                                                       unsigned long long* __restrict__ words)
{
  int bad = 0;
  // (n < 2^29: 3 i fits 32 bits)
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < (unsigned)n; i += gridDim.x * blockDim.x) {
    const int32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const int32_t bx = x / bin, by = y / bin;
    if (x < 0 || y < 0 || bx >= w || by >= h) {
      bad = 1;
      continue;
    }
    bool counts = !rule.below(x, y, z, ground_th);
    const int32_t lab = plane_idx[i];
    const bool planar = lab >= 1 && lab <= n_planes && (!ok || ok[lab - 1]);
    const long long pix = (long long)by * w + bx;
    // (every ballot below is over the lanes that reached this line, and what it returns is the same in all of them.  The
    // lane after this one may not have reached it -- a point outside the lattice, or past n -- and `next` is then undefined:
    // it only feeds the choice between two forms that give the same sums, made by the whole wave alike)
    const long long next = __shfl_down(pix, 1);
    if (__popcll(__ballot(counts && pix == next)) < AGG_MIN) {
      if (counts)
        atomicAdd(packed + pix, 1ull | ((unsigned long long)planar << 32));
      continue;
    }
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(counts);
    while (todo) {  // one add per distinct pixel of the wave, by the first lane that holds it
      const int leader = __ffsll((long long)todo) - 1;
      const long long p0 = __shfl(pix, leader);
      const bool mine = counts && pix == p0;
      const unsigned long long m = __ballot(mine), pm = __ballot(mine && planar);
      if (lane == leader)
        atomicAdd(packed + p0, (unsigned long long)__popcll(m) | ((unsigned long long)__popcll(pm) << 32));
      todo &= ~m;
      if (mine)
        counts = false;
    }
  }
  if (bad)
    atomicOr(words + M_RANGE, 1ull);
}

// ---- 2. window sums, keep, figures ----------------------------------------------------------------------------------------
// The window sums of one line of `len` entries (stride `step`) in place: v[o] becomes v[o] + .. + v[o + 2r] for o < outputs.
// v[o] is read before it is written and every later read is at a higher index.
__device__ inline void running_window(int32_t* v, int step, int len, int outputs, int r)
{
  int32_t s = 0;
  for (int j = 0; j <= 2 * r; j++)
    s += v[j * step];
  for (int o = 0; o < outputs; o++) {
    const int32_t first = v[o * step];
    v[o * step] = s;
    const int next = o + 2 * r + 1;
    s += (next < len ? v[next * step] : 0) - first;
  }
}

__global__ __launch_bounds__(256) void ev_window_kernel(const unsigned long long* __restrict__ packed, int32_t w, int32_t h,
                                                        int32_t r, int32_t min_points, int32_t num, int32_t den,
                                                        long long n_tiles, int32_t tiles_x, uint8_t* __restrict__ keep,
                                                        int32_t* __restrict__ above_out, int32_t* __restrict__ planar_out,
                                                        int32_t* __restrict__ win_above, int32_t* __restrict__ win_planar,
                                                        unsigned long long* __restrict__ words)
{
  __shared__ int32_t s_a[LW * LS], s_p[LW * LS];
  __shared__ unsigned long long s_fig[M_WORDS];
  if (threadIdx.x < M_WORDS)
    s_fig[threadIdx.x] = 0;
  const int lw = TILE + 2 * r;  // the LDS tile is lw x lw
  unsigned long long f_counted = 0, f_planar = 0;
  unsigned f_pixels = 0, f_kept = 0, f_rejected = 0, f_thin = 0;
  int32_t f_max = 0;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long long ty = t / tiles_x;
    const int32_t x0 = (int32_t)(t - ty * tiles_x) * TILE, y0 = (int32_t)ty * TILE;
    __syncthreads();  // (the tile before is read no more; s_fig is zeroed)
    for (int j = threadIdx.x; j < lw * lw; j += 256) {
      const int ly = j / lw, lx = j - ly * lw;
      const int32_t gx = x0 - r + lx, gy = y0 - r + ly;
      unsigned long long v = 0;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h)
        v = packed[(long long)gy * w + gx];
      s_a[ly * LS + lx] = (int32_t)(v & 0xffffffffull);
      s_p[ly * LS + lx] = (int32_t)(v >> 32);
    }
    __syncthreads();
    // along x: a thread per row and plane
    if ((int)threadIdx.x < 2 * lw) {
      const int row = threadIdx.x >> 1;
      running_window(((threadIdx.x & 1) ? s_p : s_a) + row * LS, 1, lw, TILE, r);
    }
    __syncthreads();
    // along y: a thread per output column and plane
    if (threadIdx.x < 2 * TILE) {
      const int col = threadIdx.x & (TILE - 1);
      running_window(((int)threadIdx.x >= TILE ? s_p : s_a) + col, LS, lw, TILE, r);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < TILE * TILE; j += 256) {
      const int oy = j / TILE, ox = j - oy * TILE;
      const int32_t gx = x0 + ox, gy = y0 + oy;
      if (gx >= w || gy >= h)
        continue;
      const long long pix = (long long)gy * w + gx;
      const int32_t A = s_a[oy * LS + ox], P = s_p[oy * LS + ox];
      const unsigned long long own = packed[pix];
      const int32_t a = (int32_t)(own & 0xffffffffull), p = (int32_t)(own >> 32);
      const bool enough = A >= min_points;
      const bool share = (long long)P * den >= (long long)num * A;
      keep[pix] = enough && share;
      if (above_out)
        above_out[pix] = a;
      if (planar_out)
        planar_out[pix] = p;
      if (win_above)
        win_above[pix] = A;
      if (win_planar)
        win_planar[pix] = P;
      f_counted += (unsigned)a;
      f_planar += (unsigned)p;
      f_pixels += a > 0;
      f_kept += enough && share;
      f_rejected += enough && !share;
      f_thin += A > 0 && !enough;
      f_max = max(f_max, A);
    }
  }
  unsigned long long v[M_WORDS] = {0, f_counted, f_planar, f_pixels, f_kept, f_rejected, f_thin, 0};
  for (int o = 32; o > 0; o >>= 1) {
    for (int k = M_COUNTED; k < M_MAX; k++)
      v[k] += __shfl_xor(v[k], o);
    f_max = max(f_max, __shfl_xor(f_max, o));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    for (int k = M_COUNTED; k < M_MAX; k++)
      if (v[k])
        atomicAdd(&s_fig[k], v[k]);
    atomicMax(&s_fig[M_MAX], (unsigned long long)f_max);
  }
  __syncthreads();
  if (threadIdx.x >= M_COUNTED && threadIdx.x < M_MAX && s_fig[threadIdx.x])
    atomicAdd(words + threadIdx.x, s_fig[threadIdx.x]);
  if (threadIdx.x == M_MAX && s_fig[M_MAX])
    atomicMax(words + M_MAX, s_fig[M_MAX]);
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct Args {
  int32_t n_planes, bin, r, min_points, num, den, width, height;
  double ground_th;
};

int check_args(bs_ctx* ctx, const void* xyz, int64_t n, const void* plane_idx, int32_t n_planes, const int32_t* extent,
               int32_t bin, int32_t r, int32_t min_points, int32_t num, int32_t den, const void* keep, const void* out,
               int32_t* width, int32_t* height)
{
  if (!xyz || !plane_idx || !extent || !keep || !out)
    return fail(ctx, BS_ERR_INVALID, "roof evidence: null pointer");
  if (n < 1 || bin < 1 || n_planes < 0)
    return fail(ctx, BS_ERR_INVALID, "roof evidence: n < 1, bin < 1 or n_planes < 0");
  if (bs_grid_dims(extent, bin, width, height) != BS_OK)
    return fail(ctx, BS_ERR_INVALID, "roof evidence: bad extent");
  if (r < 0 || r > RMAX || min_points < 1 || den < 1 || num < 0 || num > den)
    return fail(ctx, BS_ERR_INVALID, "roof evidence: r outside 0 .. 15, min_points < 1, den < 1 or num outside 0 .. den");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "roof evidence: 2^29 points or more");
  if ((long long)*width * *height >= (1ll << 31) - 1)
    return fail(ctx, BS_ERR_RANGE, "roof evidence: 2^31 - 1 pixels or more");
  return BS_OK;
}

// the stage on a device cloud; res is zeroed; d_keep is written, every other image where it is given
int evidence(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* d_plane_idx, const uint8_t* plane_ok, const Args& a,
             uint8_t* d_keep, int32_t* d_above, int32_t* d_planar, int32_t* d_win_above, int32_t* d_win_planar,
             struct bs_roof_evidence& res)
{
  const int32_t w = a.width, h = a.height;
  const long long npix = (long long)w * h;
  res.width = w;
  res.height = h;
  res.r = a.r;
  res.min_points = a.min_points;
  res.num = a.num;
  res.den = a.den;
  res.grid = GRID;
  res.tile = TILE;
  res.n_points = n;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->evd;
  Events<3> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));
  BS_HIP(ctx, B[EV_MISC].reserve(8 * M_WORDS));
  BS_HIP(ctx, B[EV_PACKED].reserve(8 * (size_t)npix));
  unsigned long long* words = B[EV_MISC].as<unsigned long long>();
  unsigned long long* packed = B[EV_PACKED].as<unsigned long long>();
  const uint8_t* d_ok = nullptr;
  if (plane_ok && a.n_planes > 0) {
    BS_HIP(ctx, B[EV_OK].reserve((size_t)a.n_planes));
    BS_HIP(ctx, hipMemcpyAsync(B[EV_OK].p, plane_ok, (size_t)a.n_planes, hipMemcpyHostToDevice, st));
    d_ok = B[EV_OK].as<uint8_t>();
  }
  unsigned long long h_words[M_WORDS] = {};
  const int ngrid = (int)std::max<long long>(1, std::min<long long>(nblk(n, 256), GRID));
  const int32_t tiles_x = nblk(w, TILE), tiles_y = nblk(h, TILE);
  const long long n_tiles = (long long)tiles_x * tiles_y;
  const int wgrid = (int)std::min<long long>(n_tiles, WIN_GRID);

  // 1. counts
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(words, 0, 8 * M_WORDS, st));
  BS_HIP(ctx, hipMemsetAsync(packed, 0, 8 * (size_t)npix, st));
  ev_count_kernel<<<ngrid, 256, 0, st>>>(d_xyz, n, d_plane_idx, a.n_planes, d_ok, a.bin, w, h, a.ground_th, ground_rule(ctx),
                                         packed, words);
  BS_HIP(ctx, hipMemcpyAsync(h_words, words, 8, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the range flag, before anything of the caller's is written
  BS_HIP(ctx, hipGetLastError());
  if (h_words[M_RANGE])
    return fail(ctx, BS_ERR_RANGE, "roof evidence: a point with a negative x or y, or whose pixel lies outside the lattice");
  // 2. window sums, keep, figures
  ev_window_kernel<<<wgrid, 256, 0, st>>>(packed, w, h, a.r, a.min_points, a.num, a.den, n_tiles, tiles_x, d_keep, d_above,
                                          d_planar, d_win_above, d_win_planar, words);
  BS_HIP(ctx, hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  res.n_counted = (int64_t)h_words[M_COUNTED];
  res.n_planar = (int64_t)h_words[M_PLANAR];
  res.n_pixels = (int64_t)h_words[M_PIXELS];
  res.pixels_kept = (int64_t)h_words[M_KEPT];
  res.pixels_rejected = (int64_t)h_words[M_REJECTED];
  res.pixels_thin = (int64_t)h_words[M_THIN];
  res.max_window = (int32_t)h_words[M_MAX];
  res.ms_counts = ev.ms(0, 1);
  res.ms_window = ev.ms(1, 2);
  return BS_OK;
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" int bs_plane_quality(const struct bs_plane_fits* f, int64_t min_points, int32_t max_rms, uint8_t* ok)
{
  if (!f || f->n_planes < 0 || min_points < 0 || max_rms < 0 || max_rms > 32767)
    return BS_ERR_INVALID;
  if (f->n_planes > 0 && (!ok || !f->status || !f->n_points || !f->r_sq_sum))
    return BS_ERR_INVALID;
  for (int32_t p = 0; p < f->n_planes; p++) {
    // max_rms^2 < 2^30; the product is taken in 128 bits whatever n_points holds
    const __int128 limit = (__int128)((int64_t)max_rms * max_rms) * f->n_points[p];
    ok[p] = f->status[p] == 0 && f->n_points[p] >= min_points && (__int128)f->r_sq_sum[p] <= limit;
  }
  return BS_OK;
}

extern "C" int bs_roof_evidence_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* d_plane_idx, int32_t n_planes,
                                    const uint8_t* plane_ok, const int32_t* extent, int32_t bin, double ground_th, int32_t r,
                                    int32_t min_points, int32_t num, int32_t den, uint8_t* d_keep, int32_t* d_above,
                                    int32_t* d_planar, int32_t* d_win_above, int32_t* d_win_planar,
                                    struct bs_roof_evidence* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  Args a{n_planes, bin, r, min_points, num, den, 0, 0, ground_th};
  int rc = check_args(ctx, d_xyz, n, d_plane_idx, n_planes, extent, bin, r, min_points, num, den, d_keep, out, &a.width,
                      &a.height);
  if (rc != BS_OK)
    return rc;
  struct bs_roof_evidence res;
  memset(&res, 0, sizeof res);
  rc = evidence(ctx, d_xyz, n, d_plane_idx, plane_ok, a, d_keep, d_above, d_planar, d_win_above, d_win_planar, res);
  if (rc != BS_OK)
    return rc;
  *out = res;
  return BS_OK;
}

extern "C" int bs_roof_evidence(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* plane_idx, int32_t n_planes,
                                const uint8_t* plane_ok, const int32_t* extent, int32_t bin, double ground_th, int32_t r,
                                int32_t min_points, int32_t num, int32_t den, uint8_t* keep, int32_t* above, int32_t* planar,
                                int32_t* win_above, int32_t* win_planar, struct bs_roof_evidence* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  Args a{n_planes, bin, r, min_points, num, den, 0, 0, ground_th};
  int rc = check_args(ctx, xyz, n, plane_idx, n_planes, extent, bin, r, min_points, num, den, keep, out, &a.width, &a.height);
  if (rc != BS_OK)
    return rc;
  struct bs_roof_evidence res;
  memset(&res, 0, sizeof res);
  DevBuf* B = ctx->evd;
  const size_t np = (size_t)a.width * (size_t)a.height, nn = (size_t)n;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(B[EV_IN_XYZ], xyz, 3 * nn);
  const int32_t* d_plane = S.upload(B[EV_IN_PLANE], plane_idx, nn);
  uint8_t* d_keep = S.room<uint8_t>(B[EV_KEEP], np);
  int32_t* d_above = S.room<int32_t>(B[EV_ABOVE], np, above != nullptr);
  int32_t* d_planar = S.room<int32_t>(B[EV_PLANAR], np, planar != nullptr);
  int32_t* d_win_above = S.room<int32_t>(B[EV_WIN_ABOVE], np, win_above != nullptr);
  int32_t* d_win_planar = S.room<int32_t>(B[EV_WIN_PLANAR], np, win_planar != nullptr);
  if (!S.ok())
    return S.status();
  rc = evidence(ctx, d_xyz, n, d_plane, plane_ok, a, d_keep, d_above, d_planar, d_win_above, d_win_planar, res);
  if (rc != BS_OK)
    return rc;
  S.download(keep, d_keep, np);
  S.download(above, d_above, np);
  S.download(planar, d_planar, np);
  S.download(win_above, d_win_above, np);
  S.download(win_planar, d_win_planar, np);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  *out = res;
  return BS_OK;
}
