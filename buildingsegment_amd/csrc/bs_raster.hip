// bs_raster.hip -- the reference's 2-D branch: density / height
// raster of the shifted cloud, bit-identical to buildingSeg::groundTH +
// compute_gird_picture (/root/reference/tmc3/TMC3.cpp:123-174,183-199).
//
// The reference splats every point at or above the ground threshold bilinearly
// into 4 pixels of a 100-mm grid, accumulating f64 sums IN POINT ORDER; those
// sums are order dependent, so atomics on doubles cannot reproduce them.  The
// device path makes the order explicit instead:
//   1. z histogram (integer atomics, order free) -> ground threshold
//   2. one (pixel, 4*i + corner) pair per contribution, pixel = npix for points
//      below the threshold; per-pixel counts with integer atomics
//   3. stable LSD radix sort of the pairs by pixel (rocPRIM via hipCUB): inside a
//      pixel the contributions stay in point order
//   4. one thread per pixel walks its segment sequentially with the reference's
//      own f64 expressions (no FMA), then the two per-pixel passes (mean height,
//      log density + 20) with the shared deterministic log of bs_detmath.h.
// HBM-bound helper work: 12 B/pt read + 64 B/pt of sort traffic per radix pass.
//
// There is one code path: grid_picture_tiles_dev builds the rasters of a batch of tiles
// (DESIGN.md §4 "Batches of rasters and footprints"), and the solo call
// bs_grid_picture_dev is that batch with one tile.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>

#include "../../include/bs_detmath.h"
#include "bs_common.h"
#include "bs_host.h"

namespace bs {
namespace {

constexpr int ZH_LDS = 4096;
constexpr int ZH_PER_THREAD = 32;

__global__ void accumulate_kernel(const int32_t* __restrict__ xyz, int bin, uint32_t npix,
                                  const int* __restrict__ off, const int* __restrict__ cnt,
                                  const uint32_t* __restrict__ vals, double* __restrict__ image)
{
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix)
    return;
  double c0 = 0.0, c1 = 0.0;
  const int e0 = off[p], e1 = e0 + cnt[p];
  for (int e = e0; e < e1; e++) {
    const uint32_t v = vals[e];
    const int64_t i = v >> 2;
    const int xi = (v >> 1) & 1, yi = v & 1;
    const int px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
    const int x = px / bin, y = py / bin;
    const double w = 1.0 * px / bin - x;  // TMC3.cpp:136-137
    const double h = 1.0 * py / bin - y;
    const double s = ((xi == 1) ? w : (1 - w)) * ((yi == 1) ? h : (1 - h));
    c1 += s;       // TMC3.cpp:139
    c0 += s * pz;  // TMC3.cpp:140
  }
  if (c1 != 0)  // mean height, TMC3.cpp:148-153
    c0 = c0 / c1;
  c1 = bs_det_log(c1 + 1);  // TMC3.cpp:155-160
  if (c1 != 0)
    c1 += 20;
  image[3 * (int64_t)p] = c0;
  image[3 * (int64_t)p + 1] = c1;
  image[3 * (int64_t)p + 2] = 0.0;
}

// Tile t owns points [begin, end) of the concatenation, pixels [pix, pix + W*H) of the batch image and height bins
// [hoff, hoff + nb) of one histogram.  A pair's key is pix + the pixel inside its tile and the sentinel is the batch's
// pixel count; points are tile-major, so the stable sort keeps every pixel's contributions in point order and
// accumulate_kernel walks each pixel as the reference does, whatever tiles lie around it.  A solo call is the batch
// of one tile: begin = pix = hoff = 0.
struct RasterTile {
  int64_t hoff, nb;  // height bins
  int32_t begin, end;
  int32_t width;
  uint32_t pix;
  int32_t ext[3];
  int32_t pad_;
};

struct ZBlock {  // up to 256 * ZH_PER_THREAD points of ONE tile: the block's LDS histogram is that tile's
  int32_t tile, begin, end;
};

// Height histogram.  A city block has a few dozen 1000-mm height bins: global atomics
// on so few addresses serialise in L2 (10 M points: 18 ms), so every block counts in
// LDS first and flushes its non-zero bins once (bins >= ZH_LDS go to HBM directly).
// A point outside its tile's extent is not the shifted cloud that extent belongs to
// (its splat would leave the image): it is not counted and fails the call.
__global__ __launch_bounds__(256) void zhist_tiled_kernel(const int32_t* __restrict__ xyz,
                                                          const ZBlock* __restrict__ blk,
                                                          const RasterTile* __restrict__ tiles, int bin_height,
                                                          int* __restrict__ hist, int* __restrict__ bad)
{
  __shared__ int lh[ZH_LDS];
  const ZBlock b = blk[blockIdx.x];
  const RasterTile T = tiles[b.tile];
  const int nl = (int)(T.nb < ZH_LDS ? T.nb : ZH_LDS);
  int* th = hist + T.hoff;
  for (int k = threadIdx.x; k < nl; k += blockDim.x)
    lh[k] = 0;
  __syncthreads();
  for (int64_t i = b.begin + (int64_t)threadIdx.x; i < b.end; i += blockDim.x) {
    const int x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (x < 0 || y < 0 || z < 0 || x > T.ext[0] || y > T.ext[1] || z > T.ext[2]) {
      atomicMin(bad, b.tile);  // the smallest failing tile is reported
      continue;
    }
    const int k = z / bin_height;
    if (k < ZH_LDS)
      atomicAdd(&lh[k], 1);
    else
      atomicAdd(&th[k], 1);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nl; k += blockDim.x)
    if (lh[k])
      atomicAdd(&th[k], lh[k]);
}

// groundTH (TMC3.cpp:183-199) per tile: first height bin at which the running count exceeds n_t / 2
__global__ void ground_th_tiled_kernel(const int* __restrict__ hist, const RasterTile* __restrict__ tiles,
                                       int32_t n_tiles, int bin_height, double* __restrict__ th)
{
  const int32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tiles)
    return;
  const RasterTile T = tiles[t];
  const int TH = (int)((int64_t)(T.end - T.begin) / 2);
  const int* h = hist + T.hoff;
  int total = 0;
  int64_t b;
  for (b = 0; b < T.nb; b++) {
    total += h[b];
    if (total > TH)
      break;
  }
  th[t] = (double)(int)(b * bin_height);
}

__global__ void emit_pairs_tiled_kernel(const int32_t* __restrict__ xyz, int64_t n, const int32_t* __restrict__ off,
                                        int32_t n_tiles, const RasterTile* __restrict__ tiles, int bin, uint32_t npix,
                                        const double* __restrict__ th, GroundRule rule, uint32_t* __restrict__ keys,
                                        uint32_t* __restrict__ vals, int* __restrict__ cnt)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t t = tile_of(off, n_tiles, i);
  const RasterTile T = tiles[t];
  const int px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
  // a point outside its tile's extent fails the call (zhist_tiled_kernel); it must not splat into a neighbour
  // tile or past the end of cnt
  const bool inside = px >= 0 && py >= 0 && pz >= 0 && px <= T.ext[0] && py <= T.ext[1] && pz <= T.ext[2];
  const bool keep = inside && !rule.below(px, py, pz, th[t]);  // TMC3.cpp:134
  const int x = px / bin, y = py / bin;
#pragma unroll
  for (int c = 0; c < 4; c++) {  // c = 2*xi + yi: the reference's loop order (TMC3.cpp:131-132)
    const int xi = c >> 1, yi = c & 1;
    const uint32_t pix = T.pix + (uint32_t)((int64_t)(y + yi) * T.width + (x + xi));
    keys[4 * i + c] = keep ? pix : npix;
    vals[4 * i + c] = (uint32_t)(4 * i + c);
    if (keep)
      atomicAdd(&cnt[pix], 1);
  }
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" int bs_grid_dims(const int32_t* extent, int32_t bin, int32_t* width, int32_t* height)
{
  if (!extent || !width || !height || bin <= 0 || extent[0] < 0 || extent[1] < 0)
    return BS_ERR_INVALID;
  *width = extent[0] / bin + 2;   // TMC3.cpp:75
  *height = extent[1] / bin + 2;  // TMC3.cpp:76
  return BS_OK;
}

extern "C" int bs_grid_dims_batch(const int32_t* extent, int32_t n_tiles, int32_t bin, int32_t* width, int32_t* height,
                                  int64_t* pixel_offset)
{
  if (!extent || !width || !height || !pixel_offset || n_tiles < 1)
    return BS_ERR_INVALID;
  pixel_offset[0] = 0;
  for (int32_t t = 0; t < n_tiles; t++) {
    if (bs_grid_dims(extent + 3 * (int64_t)t, bin, width + t, height + t) != BS_OK)
      return BS_ERR_INVALID;
    pixel_offset[t + 1] = pixel_offset[t] + (int64_t)width[t] * height[t];
  }
  return BS_OK;
}

namespace {

// the per-tile descriptors of a batch raster, with the parameter checks per tile (errors name the tile; the solo
// call has made the same checks in its own words before it gets here, so none of these texts reaches a solo caller:
// a check added here must be mirrored in bs_grid_picture_dev)
int raster_tiles(bs_ctx* ctx, const int64_t* off, int32_t n_tiles, const int32_t* extent, int32_t bin,
                 int32_t bin_height, std::vector<RasterTile>& tl, int64_t* npix, int64_t* nbins)
{
  if (!extent || bin <= 0 || bin_height <= 0)
    return fail(ctx, BS_ERR_INVALID, "raster batch: null extent or bad bin / bin_height");
  tl.assign(n_tiles, RasterTile{});
  int64_t np = 0, nb = 0;
  for (int32_t t = 0; t < n_tiles; t++) {
    const int32_t* e = extent + 3 * (int64_t)t;
    int32_t w = 0, h = 0;
    if (bs_grid_dims(e, bin, &w, &h) != BS_OK || e[2] < 0) {
      char msg[128];
      snprintf(msg, sizeof msg, "tile %d: bad extent (%d, %d, %d)", t, e[0], e[1], e[2]);
      return fail(ctx, BS_ERR_INVALID, msg);
    }
    RasterTile& T = tl[t];
    T.begin = (int32_t)off[t];
    T.end = (int32_t)off[t + 1];
    T.width = w;
    T.pix = (uint32_t)std::min<int64_t>(np, UINT32_MAX);
    T.hoff = nb;
    T.nb = (int64_t)e[2] / bin_height + 1;
    for (int a = 0; a < 3; a++)
      T.ext[a] = e[a];
    np += (int64_t)w * h;
    nb += T.nb;
  }
  if (np >= (1ll << 31) - 1)
    return fail(ctx, BS_ERR_RANGE, "raster batch: 2^31 - 1 pixels or more in all");
  *npix = np;
  *nbins = nb;
  return BS_OK;
}

int check_raster_points(bs_ctx* ctx, const int64_t* off, int32_t n_tiles, int64_t* n)
{
  if (off && n_tiles >= 1 && off[n_tiles] >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "raster batch: 2^29 points or more in all");
  return check_tiles(ctx, off, n_tiles, 1, n);
}

// The rasters of n_tiles tiles in one pass; the callers have checked tile_offset and the pointers.  A point outside
// its tile's extent sets *bad_tile to the smallest such tile and returns BS_ERR_RANGE; the caller words the message.
int grid_picture_tiles_dev(bs_ctx* ctx, const int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                           const int32_t* extent, int32_t bin, int32_t bin_height, double* d_image, double* ground_th,
                           int32_t* bad_tile)
{
  *bad_tile = -1;
  const int64_t n = tile_offset[n_tiles];
  int64_t npix64 = 0, nb = 0;
  std::vector<RasterTile> tl;
  int rc = raster_tiles(ctx, tile_offset, n_tiles, extent, bin, bin_height, tl, &npix64, &nb);
  if (rc != BS_OK)
    return rc;
  const uint32_t npix = (uint32_t)npix64;
  std::vector<ZBlock> blk;
  const int64_t chunk = 256 * ZH_PER_THREAD;
  for (int32_t t = 0; t < n_tiles; t++)
    for (int64_t b = tile_offset[t]; b < tile_offset[t + 1]; b += chunk)
      blk.push_back({t, (int32_t)b, (int32_t)std::min<int64_t>(tile_offset[t + 1], b + chunk)});
  // descriptors: RasterTile [n_tiles] | offsets int32 [n_tiles + 1] | ZBlock [blocks]
  const size_t d_tiles = sizeof(RasterTile) * n_tiles, d_off = sizeof(int32_t) * (n_tiles + 1);
  std::vector<char> desc(d_tiles + d_off + sizeof(ZBlock) * blk.size());
  memcpy(desc.data(), tl.data(), d_tiles);
  for (int32_t t = 0; t <= n_tiles; t++) {
    const int32_t o = (int32_t)tile_offset[t];
    memcpy(desc.data() + d_tiles + sizeof(int32_t) * t, &o, sizeof o);
  }
  memcpy(desc.data() + d_tiles + d_off, blk.data(), sizeof(ZBlock) * blk.size());
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  BS_HIP(ctx, ctx->tile_desc.reserve(desc.size()));
  const RasterTile* dt = ctx->tile_desc.as<RasterTile>();
  const int32_t* doff = reinterpret_cast<const int32_t*>(ctx->tile_desc.as<char>() + d_tiles);
  const ZBlock* dblk = reinterpret_cast<const ZBlock*>(ctx->tile_desc.as<char>() + d_tiles + d_off);
  BS_HIP(ctx, hipMemcpyAsync(ctx->tile_desc.p, desc.data(), desc.size(), hipMemcpyHostToDevice, st));

  const int64_t m = 4 * n;
  BS_HIP(ctx, ctx->rs_keys_in.reserve(sizeof(uint32_t) * m));
  BS_HIP(ctx, ctx->rs_keys_out.reserve(sizeof(uint32_t) * m));
  BS_HIP(ctx, ctx->rs_vals_in.reserve(sizeof(uint32_t) * m));
  BS_HIP(ctx, ctx->rs_vals_out.reserve(sizeof(uint32_t) * m));
  // cnt[npix] | off[npix] | hist[nb] | bad | pad | th[n_tiles] (doubles, 8-aligned)
  const size_t ints = (size_t)2 * npix + (size_t)nb + 1;
  const size_t th_off = ((ints * sizeof(int) + 7) / 8) * 8;
  BS_HIP(ctx, ctx->rs_cnt.reserve(th_off + sizeof(double) * n_tiles));
  int* cnt = ctx->rs_cnt.as<int>();
  int* off = cnt + npix;
  int* hist = off + npix;
  int* bad = hist + nb;
  double* d_th = reinterpret_cast<double*>(ctx->rs_cnt.as<char>() + th_off);
  BS_HIP(ctx, hipMemsetAsync(cnt, 0, th_off + sizeof(double) * n_tiles, st));
  BS_HIP(ctx, hipMemsetAsync(bad, 0x7f, sizeof(int), st));  // INT32 above every tile index: no failing tile

  zhist_tiled_kernel<<<(int)blk.size(), 256, 0, st>>>(d_xyz, dblk, dt, bin_height, hist, bad);
  ground_th_tiled_kernel<<<nblk(n_tiles, 64), 64, 0, st>>>(hist, dt, n_tiles, bin_height, d_th);
  uint32_t* keys_in = ctx->rs_keys_in.as<uint32_t>();
  uint32_t* vals_in = ctx->rs_vals_in.as<uint32_t>();
  uint32_t* keys_out = ctx->rs_keys_out.as<uint32_t>();
  uint32_t* vals_out = ctx->rs_vals_out.as<uint32_t>();
  emit_pairs_tiled_kernel<<<nblk(n, 256), 256, 0, st>>>(d_xyz, n, doff, n_tiles, dt, bin, npix, d_th, ground_rule(ctx), keys_in,
                                                        vals_in, cnt);
  int end_bit = 1;
  while (end_bit < 32 && (1ull << end_bit) <= (unsigned long long)npix)
    end_bit++;
  auto sort = [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (int)m, 0, end_bit, st);
  };
  auto scan = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, cnt, off, (int)npix, st); };
  BS_HIP(ctx, cub_room(ctx->rs_tmp, sort, scan));
  BS_HIP(ctx, cub_run(ctx->rs_tmp, sort));
  BS_HIP(ctx, cub_run(ctx->rs_tmp, scan));
  accumulate_kernel<<<nblk(npix, 64), 64, 0, st>>>(d_xyz, bin, npix, off, cnt, vals_out, d_image);
  int h_bad = 0;
  std::vector<double> h_th(n_tiles);
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_th.data(), d_th, sizeof(double) * n_tiles, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_bad != 0x7f7f7f7f) {
    *bad_tile = h_bad;
    return BS_ERR_RANGE;
  }
  if (ground_th)
    memcpy(ground_th, h_th.data(), sizeof(double) * n_tiles);
  return BS_OK;
}

}  // namespace

extern "C" int bs_grid_picture_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* extent, int32_t bin,
                                   int32_t bin_height, double* d_image, double* ground_th)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int32_t width = 0, height = 0;
  if (!d_xyz || !d_image || n <= 0 || bin_height <= 0 || bs_grid_dims(extent, bin, &width, &height) != BS_OK ||
      extent[2] < 0)
    return fail(ctx, BS_ERR_INVALID, "null pointer, empty cloud or bad raster parameters");
  if (n >= (1ll << 29) || (int64_t)width * height >= (1ll << 31) - 1)
    return fail(ctx, BS_ERR_RANGE, "raster: more than 2^29 points or 2^31 pixels");
  const int64_t off[2] = {0, n};
  int32_t bad_tile = -1;
  const int rc = grid_picture_tiles_dev(ctx, d_xyz, off, 1, extent, bin, bin_height, d_image, ground_th, &bad_tile);
  if (bad_tile >= 0)
    return fail(ctx, BS_ERR_RANGE, "raster: a coordinate lies outside [0, extent] (cloud not shifted to its bounding box?)");
  return rc;
}

extern "C" int bs_grid_picture(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* extent, int32_t bin,
                               int32_t bin_height, double* image, double* ground_th)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int32_t width = 0, height = 0;
  if (!xyz || !image || n <= 0 || bs_grid_dims(extent, bin, &width, &height) != BS_OK)
    return fail(ctx, BS_ERR_INVALID, "null pointer, empty cloud or bad raster parameters");
  Staging S(ctx);
  const size_t img = 3 * (size_t)width * height;
  const int32_t* d_xyz = S.upload(ctx->d_xyz_h, xyz, 3 * n);
  double* d_image = S.room<double>(ctx->rs_img, img);
  if (!S.ok())
    return S.status();
  const int rc = bs_grid_picture_dev(ctx, d_xyz, n, extent, bin, bin_height, d_image, ground_th);
  if (rc != BS_OK)
    return rc;
  S.download(image, d_image, img);
  return S.finish();
}

extern "C" int bs_grid_picture_batch_dev(bs_ctx* ctx, const int32_t* d_xyz, const int64_t* tile_offset,
                                         int32_t n_tiles, const int32_t* extent, int32_t bin, int32_t bin_height,
                                         double* d_image, double* ground_th)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int64_t n = 0;
  int rc = check_raster_points(ctx, tile_offset, n_tiles, &n);
  if (rc != BS_OK)
    return rc;
  if (!d_xyz || !d_image)
    return fail(ctx, BS_ERR_INVALID, "raster batch: null device pointer");
  if (ctx->gm_on && n_tiles > 1)
    return fail(ctx, BS_ERR_INVALID, "raster batch: more than one tile while a ground model is set (bs_set_ground_model)");
  int32_t bad_tile = -1;
  rc = grid_picture_tiles_dev(ctx, d_xyz, tile_offset, n_tiles, extent, bin, bin_height, d_image, ground_th,
                              &bad_tile);
  if (bad_tile >= 0) {
    char msg[160];
    snprintf(msg, sizeof msg, "raster batch: tile %d has a coordinate outside [0, extent] (not shifted to its "
                              "bounding box?)", bad_tile);
    return fail(ctx, BS_ERR_RANGE, msg);
  }
  return rc;
}

extern "C" int bs_grid_picture_batch(bs_ctx* ctx, const int32_t* xyz, const int64_t* tile_offset, int32_t n_tiles,
                                     const int32_t* extent, int32_t bin, int32_t bin_height, double* image,
                                     double* ground_th)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int64_t n = 0, npix = 0, nb = 0;
  int rc = check_raster_points(ctx, tile_offset, n_tiles, &n);
  if (rc != BS_OK)
    return rc;
  if (!xyz || !image)
    return fail(ctx, BS_ERR_INVALID, "raster batch: null host pointer");
  if (ctx->gm_on && n_tiles > 1)
    return fail(ctx, BS_ERR_INVALID, "raster batch: more than one tile while a ground model is set (bs_set_ground_model)");
  std::vector<RasterTile> tl;
  rc = raster_tiles(ctx, tile_offset, n_tiles, extent, bin, bin_height, tl, &npix, &nb);
  if (rc != BS_OK)
    return rc;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(ctx->d_xyz_h, xyz, 3 * n);
  double* d_image = S.room<double>(ctx->rs_img, 3 * (size_t)npix);
  if (!S.ok())
    return S.status();
  rc = bs_grid_picture_batch_dev(ctx, d_xyz, tile_offset, n_tiles, extent, bin, bin_height, d_image, ground_th);
  if (rc != BS_OK)
    return rc;
  S.download(image, d_image, 3 * (size_t)npix);
  return S.finish();
}
