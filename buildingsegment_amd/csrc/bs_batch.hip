// bs_batch.hip -- n_tiles independent clouds in one device pass (bs_segment_batch[_dev], bs_batch_planes_fetch,
// bs_shift_tiles_to_origin_dev, bs_tile_boxes_dev; declarations: include/bs_api.h, argument: DESIGN.md §4 "Batches of
// tiles").
//
// The grid (bs_grid.hip, build_grid_tiled) and the kNN (bs_knn.hip, TILED instances) never let a query see another
// tile, so every neighbour row holds indices of its own tile, in the concatenation's numbering.  The growers then run
// unchanged over the concatenation: the sequential rule visits seeds in index order and a plane only ever takes points
// reachable through rows of its seed's tile, so tile t's planes are exactly its solo planes, committed as one
// contiguous run of the global plane counter starting at base[t] + 1, where base[t] = the number of committed seeds
// below tile_offset[t].  What is left is renumbering: rows minus the tile's offset, labels minus base[t], plane ids
// minus base[t] and plane lists minus the tile's offset.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "bs_host.h"

namespace bs {

namespace {

// base[t] = committed planes whose seed lies below off[t] (t = 0 .. n_tiles); the records are in commit order, which
// is ascending seed order
__global__ void plane_base_kernel(const PlaneRec* __restrict__ recs, const GrowStats* __restrict__ stats,
                                  const int32_t* __restrict__ off, int32_t n_tiles, int32_t* __restrict__ base)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > n_tiles)
    return;
  const int32_t v = off[t];
  int32_t lo = 0, hi = stats->n_planes;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (recs[mid].seed < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  base[t] = lo;
}

__global__ void rows_local_kernel(int32_t* __restrict__ neigh, int64_t n, int K, const int32_t* __restrict__ off,
                                  int32_t n_tiles)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t o = off[tile_of(off, n_tiles, i)];
  int32_t* row = neigh + i * K;
  for (int j = 0; j < K; j++)
    row[j] -= o;
}

__global__ void labels_local_kernel(int32_t* __restrict__ plane_idx, int64_t n, const int32_t* __restrict__ off,
                                    int32_t n_tiles, const int32_t* __restrict__ base)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t l = plane_idx[i];
  if (l >= 1)
    plane_idx[i] = l - base[tile_of(off, n_tiles, i)];
}

// plane p (0-based) belongs to the last tile t with base[t] <= p
__global__ void recs_local_kernel(const PlaneRec* __restrict__ recs, const GrowStats* __restrict__ stats,
                                  const int32_t* __restrict__ base, int32_t n_tiles, PlaneRec* __restrict__ out)
{
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= stats->n_planes)
    return;
  PlaneRec r = recs[p];
  r.id = p + 1 - base[tile_of(base, n_tiles, p)];
  out[p] = r;
}

// every entry of a plane list is a point of the plane's tile
__global__ void list_local_kernel(const int32_t* __restrict__ list, const GrowStats* __restrict__ stats,
                                  const int32_t* __restrict__ off, int32_t n_tiles, int32_t* __restrict__ out)
{
  const int64_t used = stats->list_used;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < used; e += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = list[e];
    out[e] = v - off[tile_of(off, n_tiles, v)];
  }
}

inline int blocks_of(int64_t n, int bs) { return (int)std::max<int64_t>(1, (n + bs - 1) / bs); }

// the offsets as int32 on the device (BT_OFF)
int upload_offsets(bs_ctx* ctx, const std::vector<int64_t>& off)
{
  std::vector<int32_t> o32(off.begin(), off.end());
  BS_HIP(ctx, ctx->bt[BT_OFF].reserve(sizeof(int32_t) * o32.size()));
  BS_HIP(ctx, hipMemcpyAsync(ctx->bt[BT_OFF].p, o32.data(), sizeof(int32_t) * o32.size(), hipMemcpyHostToDevice,
                             ctx->stream));
  BS_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (o32 is a host temporary)
  return BS_OK;
}

struct Timer {
  bs_ctx* ctx;
  void mark(int i) { (void)hipEventRecord(ctx->ev[i], ctx->stream); }
  double ms(int i, int j)
  {
    float t = 0.f;
    return hipEventElapsedTime(&t, ctx->ev[i], ctx->ev[j]) == hipSuccess ? (double)t : 0.0;
  }
};

}  // namespace

// tile_offset checks shared by every batch entry point (bs_common.h); min_pts = k (segmentation) or 1 (shift, rasters)
int check_tiles(bs_ctx* ctx, const int64_t* off, int32_t n_tiles, int64_t min_pts, int64_t* total)
{
  char msg[160];
  if (!off)
    return fail(ctx, BS_ERR_INVALID, "tile_offset is NULL");
  if (n_tiles < 1)
    return fail(ctx, BS_ERR_INVALID, "n_tiles must be >= 1");
  if (off[0] != 0)
    return fail(ctx, BS_ERR_INVALID, "tile_offset[0] must be 0");
  for (int32_t t = 0; t < n_tiles; t++) {
    const int64_t m = off[t + 1] - off[t];
    if (m < 0) {
      snprintf(msg, sizeof msg, "tile %d: tile_offset decreases (%lld after %lld)", t, (long long)off[t + 1],
               (long long)off[t]);
      return fail(ctx, BS_ERR_INVALID, msg);
    }
    if (m < min_pts) {
      snprintf(msg, sizeof msg, "tile %d has %lld points, fewer than %lld (k; the reference is undefined there)", t,
               (long long)m, (long long)min_pts);
      return fail(ctx, BS_ERR_INVALID, msg);
    }
    if (off[t + 1] >= (int64_t)INT32_MAX - 64) {
      snprintf(msg, sizeof msg, "tile %d ends at point %lld: a batch must hold fewer than INT32_MAX - 64 points", t,
               (long long)off[t + 1]);
      return fail(ctx, BS_ERR_INVALID, msg);
    }
  }
  *total = off[n_tiles];
  return BS_OK;
}

}  // namespace bs

using namespace bs;

extern "C" {

int bs_segment_batch_dev(bs_ctx* ctx, const int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                         const bs_params* p, int32_t* d_neigh, double* d_normals, int32_t* d_plane_idx)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!p)
    return fail(ctx, BS_ERR_INVALID, "params is NULL");
  int64_t n = 0;
  int rc = check_tiles(ctx, tile_offset, n_tiles, std::max(p->k, 1), &n);
  if (rc != BS_OK)
    return rc;
  rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  if (!d_xyz || !d_plane_idx)
    return fail(ctx, BS_ERR_INVALID, "null device pointer");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  ctx->bt_valid = false;
  std::vector<int64_t> off(tile_offset, tile_offset + n_tiles + 1);
  const bool own_neigh = d_neigh != nullptr;
  if (!d_neigh) {
    BS_HIP(ctx, ctx->seg_neigh.reserve(sizeof(int32_t) * n * p->k));
    d_neigh = ctx->seg_neigh.as<int32_t>();
  }
  if (!d_normals) {
    BS_HIP(ctx, ctx->seg_normals.reserve(sizeof(double) * n * 3));
    d_normals = ctx->seg_normals.as<double>();
  }
  rc = upload_offsets(ctx, off);
  if (rc != BS_OK)
    return rc;
  const int32_t* d_off = ctx->bt[BT_OFF].as<int32_t>();
  Timer T{ctx};
  T.mark(5);
  TiledGridDev g;
  rc = build_grid_tiled(ctx, d_xyz, d_off, off, p->radius, p->k, p->cell_size, &g);
  if (rc != BS_OK)
    return rc;
  T.mark(1);
  // the fused hand-off of bs_segment_dev: neighbour positions and normals in cell-sorted order for the grower
  int32_t* d_npos = nullptr;
  if (p->rg_mode != 1) {
    BS_HIP(ctx, ctx->seg_npos.reserve(sizeof(int32_t) * ((size_t)n * p->k + 2) + sizeof(double) * 3 * (size_t)n));
    d_npos = ctx->seg_npos.as<int32_t>();
  }
  ctx->npos_neigh = nullptr;
  ctx->npos_normals = nullptr;
  rc = launch_knn_normals_tiled(ctx, g, *p, d_neigh, d_normals, d_npos);
  if (rc != BS_OK)
    return rc;
  T.mark(2);
  if (d_npos) {
    ctx->npos_neigh = d_neigh;
    ctx->npos_normals = d_normals;
    ctx->npos_k = p->k;
  }
  rc = region_grow_dev_impl(ctx, d_xyz, d_normals, d_neigh, n, p, d_plane_idx, true);
  ctx->npos_neigh = nullptr;  // the rows are renumbered below: no longer what the positions were taken from
  ctx->npos_normals = nullptr;
  if (rc != BS_OK)
    return rc;
  // renumbering: labels by the plane bases, rows by the tile offsets
  hipStream_t st = ctx->stream;
  BS_HIP(ctx, ctx->bt[BT_BASE].reserve(sizeof(int32_t) * (n_tiles + 1)));
  int32_t* d_base = ctx->bt[BT_BASE].as<int32_t>();
  plane_base_kernel<<<blocks_of(n_tiles + 1, 256), 256, 0, st>>>(ctx->rg_planes.as<PlaneRec>(),
                                                                 ctx->rg_stats.as<GrowStats>(), d_off, n_tiles, d_base);
  labels_local_kernel<<<blocks_of(n, 256), 256, 0, st>>>(d_plane_idx, n, d_off, n_tiles, d_base);
  if (own_neigh)
    rows_local_kernel<<<blocks_of(n, 256), 256, 0, st>>>(d_neigh, n, p->k, d_off, n_tiles);
  BS_HIP(ctx, hipGetLastError());
  T.mark(6);
  BS_HIP(ctx, hipEventSynchronize(ctx->ev[6]));
  ctx->tm.grid_ms = T.ms(5, 1);
  ctx->tm.knn_ms = T.ms(1, 2);
  ctx->tm.total_ms = T.ms(5, 6);
  ctx->bt_off = off;
  ctx->bt_valid = true;
  return BS_OK;
}

int bs_batch_planes_fetch(bs_ctx* ctx, bs_planes* planes, int32_t* plane_offset)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (planes)
    memset(planes, 0, sizeof *planes);
  if (!ctx->bt_valid || !ctx->rg_valid || ctx->rg_n != ctx->bt_off.back())
    return fail(ctx, BS_ERR_INVALID, "no batch result on this context (bs_segment_batch[_dev])");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int32_t nt = (int32_t)ctx->bt_off.size() - 1;
  int rc = upload_offsets(ctx, ctx->bt_off);
  if (rc != BS_OK)
    return rc;
  const int32_t* d_off = ctx->bt[BT_OFF].as<int32_t>();
  GrowStats hs;
  BS_HIP(ctx, hipMemcpyAsync(&hs, ctx->rg_stats.p, sizeof hs, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, ctx->bt[BT_BASE].reserve(sizeof(int32_t) * (nt + 1)));
  BS_HIP(ctx, ctx->bt[BT_RECS].reserve(sizeof(PlaneRec) * std::max(hs.n_planes, 1)));
  BS_HIP(ctx, ctx->bt[BT_LIST].reserve(sizeof(int32_t) * std::max<int64_t>(hs.list_used, 1)));
  int32_t* d_base = ctx->bt[BT_BASE].as<int32_t>();
  const GrowStats* d_stats = ctx->rg_stats.as<GrowStats>();
  plane_base_kernel<<<blocks_of(nt + 1, 256), 256, 0, st>>>(ctx->rg_planes.as<PlaneRec>(), d_stats, d_off, nt, d_base);
  recs_local_kernel<<<blocks_of(hs.n_planes, 256), 256, 0, st>>>(ctx->rg_planes.as<PlaneRec>(), d_stats, d_base, nt,
                                                                 ctx->bt[BT_RECS].as<PlaneRec>());
  list_local_kernel<<<(int)std::min<int64_t>(blocks_of(hs.list_used, 256), 8192), 256, 0, st>>>(
      ctx->rg_list.as<int32_t>(), d_stats, d_off, nt, ctx->bt[BT_LIST].as<int32_t>());
  BS_HIP(ctx, hipGetLastError());
  std::vector<int32_t> base(nt + 1);
  BS_HIP(ctx, hipMemcpyAsync(base.data(), d_base, sizeof(int32_t) * (nt + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  if (base[nt] != hs.n_planes)
    return fail(ctx, BS_ERR_INTERNAL, "batch: plane seeds do not cover the committed planes");
  if (plane_offset)
    memcpy(plane_offset, base.data(), sizeof(int32_t) * (nt + 1));
  if (planes)
    return planes_to_host(ctx, ctx->bt[BT_RECS].as<PlaneRec>(), ctx->bt[BT_LIST].as<int32_t>(), hs.n_planes,
                          hs.list_used, planes);
  return BS_OK;
}

int bs_segment_batch(bs_ctx* ctx, const int32_t* xyz, const int64_t* tile_offset, int32_t n_tiles, const bs_params* p,
                     int32_t* neigh, double* normals, int32_t* plane_idx, bs_planes* planes, int32_t* plane_offset)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (planes)
    memset(planes, 0, sizeof *planes);
  if (!p)
    return fail(ctx, BS_ERR_INVALID, "params is NULL");
  int64_t n = 0;
  int rc = check_tiles(ctx, tile_offset, n_tiles, std::max(p->k, 1), &n);
  if (rc != BS_OK)
    return rc;
  rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  if (!xyz || !plane_idx)
    return fail(ctx, BS_ERR_INVALID, "null host pointer");
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(ctx->d_xyz_h, xyz, 3 * n);
  int32_t* d_neigh = S.room<int32_t>(ctx->d_neigh_h, n * p->k);
  double* d_normals = S.room<double>(ctx->d_normals_h, 3 * n);
  int32_t* d_plane = S.room<int32_t>(ctx->d_plane_h, n);
  if (!S.ok())
    return S.status();
  rc = bs_segment_batch_dev(ctx, d_xyz, tile_offset, n_tiles, p, d_neigh, d_normals, d_plane);
  if (rc != BS_OK)
    return rc;
  S.download(neigh, d_neigh, n * p->k);
  S.download(normals, d_normals, 3 * n);
  S.download(plane_idx, d_plane, n);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  if (planes || plane_offset)
    return bs_batch_planes_fetch(ctx, planes, plane_offset);
  return BS_OK;
}

int bs_shift_tiles_to_origin_dev(bs_ctx* ctx, int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                                 int32_t* min_out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int64_t n = 0;
  int rc = check_tiles(ctx, tile_offset, n_tiles, 1, &n);
  if (rc != BS_OK)
    return rc;
  if (!d_xyz)
    return fail(ctx, BS_ERR_INVALID, "null device pointer");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<int64_t> off(tile_offset, tile_offset + n_tiles + 1);
  rc = upload_offsets(ctx, off);
  if (rc != BS_OK)
    return rc;
  BS_HIP(ctx, ctx->bt[BT_MNMX].reserve(sizeof(int32_t) * 6 * n_tiles));
  std::vector<int32_t> bb;
  rc = tile_bbox_dev(ctx, d_xyz, ctx->bt[BT_OFF].as<int32_t>(), off, ctx->bt[BT_MNMX].as<int32_t>(), bb);
  if (rc != BS_OK)
    return rc;
  launch_tile_shift(ctx, d_xyz, n, ctx->bt[BT_OFF].as<int32_t>(), n_tiles, ctx->bt[BT_MNMX].as<int32_t>());
  BS_HIP(ctx, hipGetLastError());
  BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (min_out)
    for (int32_t t = 0; t < n_tiles; t++)
      for (int a = 0; a < 3; a++)
        min_out[3 * t + a] = bb[6 * t + a];
  ctx->order_n = 0;  // coordinates changed: a cached cell order no longer applies
  return BS_OK;
}

int bs_tile_boxes_dev(bs_ctx* ctx, const int32_t* d_xyz, const int64_t* tile_offset, int32_t n_tiles,
                      int32_t* box_out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  int64_t n = 0;
  int rc = check_tiles(ctx, tile_offset, n_tiles, 1, &n);
  if (rc != BS_OK)
    return rc;
  if (!d_xyz || !box_out)
    return fail(ctx, BS_ERR_INVALID, "null pointer");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<int64_t> off(tile_offset, tile_offset + n_tiles + 1);
  BS_HIP(ctx, ctx->bt[BT_MNMX].reserve(sizeof(int32_t) * 6 * n_tiles));
  std::vector<int32_t> bb;
  rc = tile_bbox_dev(ctx, d_xyz, nullptr, off, ctx->bt[BT_MNMX].as<int32_t>(), bb);
  if (rc != BS_OK)
    return rc;
  memcpy(box_out, bb.data(), sizeof(int32_t) * bb.size());
  return BS_OK;
}

}  // extern "C"
