// bs_grid.hip -- search-grid build for the kNN / normal kernels (gfx950).
//
// Replaces the two nanoflann kd-tree builds the reference triggers through
// Open3D (/root/reference/tmc3/my_function.h:63 and :71) by ONE hashed uniform
// grid: points are binned into cubic cells, radix-sorted by cell key (rocPRIM
// via hipCUB as a primitive), and each occupied cell gets a 16-byte entry
// {key, start, end} in an open-addressing table.  The cell-sorted copy of the
// cloud (int4 = x,y,z,global index) is what the query kernels stream, so all
// points of a cell are one contiguous, coalesced run in HBM.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "bs_common.h"
#include "bs_host.h"

namespace bs {

namespace {

__global__ void bbox_kernel(const int32_t* __restrict__ xyz, int64_t n, int32_t* __restrict__ mnmx)
{
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      int v = xyz[3 * i + a];
      mn[a] = min(mn[a], v);
      mx[a] = max(mx[a], v);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = min(mn[a], __shfl_xor(mn[a], o));
      mx[a] = max(mx[a], __shfl_xor(mx[a], o));
    }
  }
  __shared__ int smn[3][4], smx[3][4];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      smn[a][wv] = mn[a];
      smx[a][wv] = mx[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    int m0 = smn[a][0], m1 = smx[a][0];
    for (int t = 1; t < (int)(blockDim.x >> 6); t++) {
      m0 = min(m0, smn[a][t]);
      m1 = max(m1, smx[a][t]);
    }
    atomicMin(&mnmx[a], m0);
    atomicMax(&mnmx[3 + a], m1);
  }
}

// Sort key of a cell.  The hash table is keyed by pack_cell(); the ORDER of the cells in
// the sorted copy is free (only "points of one cell are contiguous" matters).  Morton
// (Z-curve) order keeps cells that are adjacent in ANY axis close in memory, so the
// gathers of everything that walks the cell-sorted order (kNN candidates, static masks,
// reverse lists, owner passes) find their neighbours' lines in the XCD's L2; the raster
// order (x fastest) separates y/z neighbours by a whole row / layer of the scene.
__host__ __device__ inline uint32_t compact21(uint64_t v)
{
  v &= 0x1249249249249249ull;
  v = (v | (v >> 2)) & 0x10C30C30C30C30C3ull;
  v = (v | (v >> 4)) & 0x100F00F00F00F00Full;
  v = (v | (v >> 8)) & 0x1F0000FF0000FFull;
  v = (v | (v >> 16)) & 0x1F00000000FFFFull;
  v = (v | (v >> 32)) & 0x1FFFFFull;
  return (uint32_t)v;
}

__global__ void cellkey_kernel(const int32_t* __restrict__ xyz, int64_t n, int mnx, int mny, int mnz,
                               int cell, int morton, uint64_t* __restrict__ keys, int32_t* __restrict__ vals)
{
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  uint32_t cx = (uint32_t)(xyz[3 * i] - mnx) / (uint32_t)cell;
  uint32_t cy = (uint32_t)(xyz[3 * i + 1] - mny) / (uint32_t)cell;
  uint32_t cz = (uint32_t)(xyz[3 * i + 2] - mnz) / (uint32_t)cell;
  keys[i] = morton ? morton_cell(cx, cy, cz) : pack_cell(cx, cy, cz);
  if (vals)
    vals[i] = (int32_t)i;
}

__global__ void count_heads_kernel(const uint64_t* __restrict__ keys, int64_t n, unsigned long long* cnt)
{
  unsigned int local = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    local += (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
  for (int o = 32; o > 0; o >>= 1)
    local += __shfl_xor(local, o);
  __shared__ unsigned int part[4];
  if ((threadIdx.x & 63) == 0)
    part[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int t = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); k++)
      t += part[k];
    if (t)
      atomicAdd(cnt, (unsigned long long)t);
  }
}

__global__ void table_clear_kernel(CellEntry* t, uint32_t size)
{
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < size) {
    t[i].key = ~0ull;
    t[i].start = 0;
    t[i].end = 0;
  }
}

__global__ void table_insert_kernel(const uint64_t* __restrict__ ukeys, const int32_t* __restrict__ ucnt,
                                    const int32_t* __restrict__ ustart, int32_t ncell, int morton,
                                    CellEntry* table, uint32_t hmask)
{
  int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell)
    return;
  uint64_t k = ukeys[c];
  if (morton)
    k = pack_cell(compact21(k), compact21(k >> 1), compact21(k >> 2));
  uint32_t h = hash_cell(k) & hmask;
  for (;;) {
    unsigned long long prev =
        atomicCAS((unsigned long long*)&table[h].key, ~0ull, (unsigned long long)k);
    if (prev == ~0ull)
      break;
    h = (h + 1) & hmask;
  }
  table[h].start = ustart[c];
  table[h].end = ustart[c] + ucnt[c];
}

__global__ void gather_sorted_kernel(const int32_t* __restrict__ xyz, const int32_t* __restrict__ gidx,
                                     const int32_t* __restrict__ order, int64_t n, int4* __restrict__ spts)
{
  int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= n)
    return;
  int32_t i = order[s];
  int4 v;
  v.x = xyz[3 * (int64_t)i];
  v.y = xyz[3 * (int64_t)i + 1];
  v.z = xyz[3 * (int64_t)i + 2];
  v.w = gidx ? gidx[i] : i;
  spts[s] = v;
}

inline int grid_blocks(int64_t n, int bs) { return (int)((n + bs - 1) / bs); }

}  // namespace

// Bits a Morton cell key occupies when the longest axis has ext / cell + 1 cells: the radix sorts run over these only
// (33 instead of 63 bits at 50 M points: 5 instead of 8 passes).
static int morton_key_bits(int64_t ext, int cell)
{
  int bits = 1;
  while (((int64_t)1 << bits) < ext / cell + 1)
    bits++;
  return std::min(63, 3 * bits);
}

// room for the keys and values of n points, before and behind the sort, and for the few words every pass reads back
static int order_room(bs_ctx* ctx, int64_t n)
{
  BS_HIP(ctx, ctx->misc.reserve(256));
  BS_HIP(ctx, ctx->keys_in.reserve(sizeof(uint64_t) * n));
  BS_HIP(ctx, ctx->keys_out.reserve(sizeof(uint64_t) * n));
  BS_HIP(ctx, ctx->vals_in.reserve(sizeof(int32_t) * n));
  BS_HIP(ctx, ctx->vals_out.reserve(sizeof(int32_t) * n));
  return BS_OK;
}

// stable radix sort of keys_in over [0, end_bit) into keys_out; pairs: vals_in goes along into vals_out
static int sort_cells(bs_ctx* ctx, int64_t n, int end_bit, bool pairs)
{
  hipStream_t st = ctx->stream;
  uint64_t* kin = ctx->keys_in.as<uint64_t>();
  uint64_t* kout = ctx->keys_out.as<uint64_t>();
  int32_t* vin = ctx->vals_in.as<int32_t>();
  int32_t* vout = ctx->vals_out.as<int32_t>();
  if (pairs)
    BS_HIP(ctx, cub_run(ctx->cub_tmp, [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, kin, kout, vin, vout, (int)n, 0, end_bit, st);
    }));
  else
    BS_HIP(ctx, cub_run(ctx->cub_tmp, [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, kin, kout, (int)n, 0, end_bit, st);
    }));
  return BS_OK;
}

// Occupied-cell count at a trial cell size: sort the keys in keys_in over [0, end_bit) and count the distinct ones
// (synchronises).  pairs: vals_out is then what step 3 of a builder would produce at this cell size (the same keys, the
// same stable sort) -- an accepted trial is the grid's sort.  (Counting by insertion into an open-addressing table
// instead of sorting was measured: the points arrive in the caller's order, 50 M random probes into a 1 GB table take
// 4.5 ms against 2.7 ms for the radix sort -- grid stage 19.7 instead of 11.0 ms.)
static int sort_count_keys(bs_ctx* ctx, int64_t n, int end_bit, int64_t* ncell, bool pairs)
{
  hipStream_t st = ctx->stream;
  if (int rc = sort_cells(ctx, n, end_bit, pairs))
    return rc;
  unsigned long long* cnt = ctx->misc.as<unsigned long long>() + 8;
  BS_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st));
  count_heads_kernel<<<std::min(grid_blocks(n, 256), 1024), 256, 0, st>>>(ctx->keys_out.as<uint64_t>(), n, cnt);
  unsigned long long h = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h, cnt, sizeof h, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  *ncell = (int64_t)h;
  return BS_OK;
}

// BS_GRID_REUSE=0 (read in every call): no trial sorts pairs, step 3 always sorts again
static bool grid_reuse_on()
{
  const char* e = getenv("BS_GRID_REUSE");
  return !e || atoi(e) != 0;
}

// Step 2 of a builder, the cell size: >= radius so one ring certifies the hybrid search, and a density-driven size
// giving ~max(4, k/2) points per occupied cell (a hint is taken as it is).  write_keys(cell, values) launches the key
// kernel of the builder at a trial size, with the values where asked, and returns the bits its keys occupy; a trial
// runs only where fits(cell).  The first trial is usually rejected and sorts keys only.  With reuse every later trial
// writes the values and sorts pairs: if its cell size is the one the rule ends on, its output IS step 3's (Morton keys,
// the same stable sort) and step 3 is skipped.  sorted_cell: the cell size whose sorted pairs are in keys_out /
// vals_out, 0 = none.
template <class WriteKeys, class Fits>
static int trial_cell(bs_ctx* ctx, int64_t n, int64_t ext, double radius, int k, int cell_hint, bool reuse, WriteKeys&& write_keys,
                      Fits&& fits, int* cell_out, int* sorted_cell)
{
  int cell = cell_hint > 0 ? cell_hint : (int)std::max(1.0, std::ceil(radius));
  *sorted_cell = 0;
  if (cell_hint <= 0) {
    const double target = std::max(4.0, 0.5 * k);
    const int cmin = cell;
    for (int it = 0; it < 4 && fits(cell); it++) {
      int64_t nc = 0;
      const bool pairs = reuse && it >= 1;
      const int end_bit = write_keys(cell, pairs);
      if (int rc = sort_count_keys(ctx, n, end_bit, &nc, pairs))
        return rc;
      *sorted_cell = pairs ? cell : 0;
      double occ = (double)n / (double)std::max<int64_t>(nc, 1);
      if (occ >= 0.7 * target && occ <= 1.6 * target)
        break;
      double f = std::sqrt(target / occ);
      f = std::min(4.0, std::max(0.25, f));
      int ncell = (int)std::floor(cell * f + 0.5);
      ncell = std::max(ncell, cmin);
      if (ncell == cell || (int64_t)ncell > ext)
        break;
      cell = ncell;
    }
  }
  *cell_out = cell;
  return BS_OK;
}

// Steps 3 to 6 of a builder over the keys and values in keys_in / vals_in, and the fields of the result that do not
// depend on the boxes.  sorted: the last trial has sorted them at this cell size already.  morton: how the table stores
// a key (table_insert_kernel).  d_gidx: the global index of every point, or null for its position.
static int finish_grid(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_gidx, int64_t n, int end_bit, bool sorted, int morton,
                       int cell, GridDev* out)
{
  hipStream_t st = ctx->stream;
  uint64_t* kout = ctx->keys_out.as<uint64_t>();
  int32_t* vout = ctx->vals_out.as<int32_t>();
  // 3. sort (unless the last trial did at this cell size)
  if (!sorted)
    if (int rc = sort_cells(ctx, n, end_bit, true))
      return rc;

  // 4. unique cells (run-length encode), starts (exclusive scan)
  BS_HIP(ctx, ctx->uniq_keys.reserve(sizeof(uint64_t) * n));
  BS_HIP(ctx, ctx->uniq_cnt.reserve(sizeof(int32_t) * 2 * n));
  uint64_t* ukeys = ctx->uniq_keys.as<uint64_t>();
  int32_t* ucnt = ctx->uniq_cnt.as<int32_t>();
  int32_t* ustart = ucnt + n;
  int32_t* d_nruns = ctx->misc.as<int32_t>() + 32;
  BS_HIP(ctx, cub_run(ctx->cub_tmp, [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceRunLengthEncode::Encode(tmp, bytes, kout, ukeys, ucnt, d_nruns, (int)n, st);
  }));
  int32_t nruns = 0;
  BS_HIP(ctx, hipMemcpyAsync(&nruns, d_nruns, sizeof nruns, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  if (nruns <= 0)
    return fail(ctx, BS_ERR_INTERNAL, "grid: no occupied cells");
  BS_HIP(ctx, cub_run(ctx->cub_tmp, [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, ucnt, ustart, nruns, st);
  }));

  // 5. hash table
  uint32_t hs = 64;
  while (hs < (uint32_t)nruns * 2u)
    hs <<= 1;
  BS_HIP(ctx, ctx->table.reserve(sizeof(CellEntry) * (size_t)hs));
  CellEntry* table = ctx->table.as<CellEntry>();
  table_clear_kernel<<<(hs + 255) / 256, 256, 0, st>>>(table, hs);
  table_insert_kernel<<<(nruns + 255) / 256, 256, 0, st>>>(ukeys, ucnt, ustart, nruns, morton, table, hs - 1);

  // 6. cell-sorted point copy
  BS_HIP(ctx, ctx->spts.reserve(sizeof(int4) * n));
  gather_sorted_kernel<<<grid_blocks(n, 256), 256, 0, st>>>(d_xyz, d_gidx, vout, n, ctx->spts.as<int4>());
  BS_HIP(ctx, hipGetLastError());

  out->cell = cell;
  out->hmask = hs - 1;
  out->table = table;
  out->spts = ctx->spts.as<int4>();
  out->slocal = vout;
  out->n = n;
  ctx->order_n = n;  // vals_out holds the cell-sorted order of this cloud (of the concatenation, for a batch)
  ctx->order_xyz = d_xyz;
  return BS_OK;
}

// bounding box of a device-resident cloud (host result; synchronises): {min x,y,z, max x,y,z}
int bbox_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bb[6])
{
  hipStream_t st = ctx->stream;
  BS_HIP(ctx, ctx->misc.reserve(256));
  int32_t init[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
  int32_t* d_mnmx = ctx->misc.as<int32_t>();
  BS_HIP(ctx, hipMemcpyAsync(d_mnmx, init, sizeof init, hipMemcpyHostToDevice, st));
  if (n > 0)
    bbox_kernel<<<std::min(grid_blocks(n, 256), 512), 256, 0, st>>>(d_xyz, n, d_mnmx);
  BS_HIP(ctx, hipMemcpyAsync(bb, d_mnmx, 6 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  return BS_OK;
}

int build_grid(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_gidx, int64_t n, double radius,
               int k, int cell_hint, GridDev* out)
{
  if (n <= 0 || n >= (int64_t)INT_MAX - 64)
    return fail(ctx, BS_ERR_INVALID, "point count out of range");
  if (int rc = order_room(ctx, n))
    return rc;

  // 1. bounding box
  int32_t bb[6];
  if (int rc = bbox_dev(ctx, d_xyz, n, bb))
    return rc;
  // exact-arithmetic domain: moment sums stay below 2^53, d^2 keys below 2^64
  const int32_t LIM = 1 << 23;
  for (int a = 0; a < 3; a++)
    if (bb[a] <= -LIM || bb[3 + a] >= LIM)
      return fail(ctx, BS_ERR_RANGE, "coordinates must satisfy |c| < 2^23 mm (8.4 km): shift the cloud to its bounding-box origin first "
                                     "(bs_shift_to_origin_dev, or the buildingSeg constructor as TMC3.cpp:210 does)");

  // 2. cell size (every trial counts Morton cells; a single cloud's key bits are clamped, so every trial fits)
  int64_t ext = 1;
  for (int a = 0; a < 3; a++)
    ext = std::max<int64_t>(ext, (int64_t)bb[3 + a] - bb[a] + 1);
  static const int morton = []() {
    const char* e = getenv("BS_GRID_ORDER");  // developer A/B switch: "raster" restores the x-fastest cell order
    return (e && e[0] == 'r') ? 0 : 1;
  }();
  auto write_keys = [&](int c, int order, bool values) {
    cellkey_kernel<<<grid_blocks(n, 256), 256, 0, ctx->stream>>>(d_xyz, n, bb[0], bb[1], bb[2], c, order, ctx->keys_in.as<uint64_t>(),
                                                                 values ? ctx->vals_in.as<int32_t>() : nullptr);
    return order ? morton_key_bits(ext, c) : 63;
  };
  int cell = 0, sorted_cell = 0;
  if (int rc = trial_cell(ctx, n, ext, radius, k, cell_hint, morton && grid_reuse_on(),
                          [&](int c, bool values) { return write_keys(c, 1, values); }, [](int) { return true; }, &cell, &sorted_cell))
    return rc;
  while (ext / cell + 1 >= (1 << 21))
    cell *= 2;

  // 3 to 6. keys (unless the last trial wrote and sorted them at this cell size), sort, cells, table, sorted copy
  const bool sorted = sorted_cell == cell;
  const int end_bit = sorted ? 0 : write_keys(cell, morton, true);
  if (int rc = finish_grid(ctx, d_xyz, d_gidx, n, end_bit, sorted, morton, cell, out))
    return rc;
  for (int a = 0; a < 3; a++) {
    out->mn[a] = bb[a];
    out->dim[a] = (int32_t)(((int64_t)bb[3 + a] - bb[a]) / cell + 1);
  }
  return BS_OK;
}

// Spatial (Morton) order of a cloud WITHOUT a search grid: what the region grower needs when it is handed
// foreign buffers (bs_region_grow[_dev], the component-sharded stage 3) -- its records, masks, reverse lists and
// owner passes address points by their position in a spatially coherent order (bs_grow_spec.hip, "Index
// spaces"); with the identity order every neighbour is a random HBM access.  One bounding-box pass, one key
// pass, one radix sort over exactly the key bits in use.  Any int32 coordinates are admissible (no exact-moment
// domain here: only an order is produced).  Result: ctx->vals_out = original index of every position.
int build_spatial_order(bs_ctx* ctx, const int32_t* d_xyz, int64_t n)
{
  if (n <= 0 || n >= (int64_t)INT_MAX - 64)
    return fail(ctx, BS_ERR_INVALID, "point count out of range");
  if (int rc = order_room(ctx, n))
    return rc;
  int32_t bb[6];
  if (int rc = bbox_dev(ctx, d_xyz, n, bb))
    return rc;
  int64_t ext = 1;
  for (int a = 0; a < 3; a++)
    ext = std::max<int64_t>(ext, (int64_t)bb[3 + a] - bb[a] + 1);
  // cells of >= 128 mm (a few points each at the densities of SURVEY 8(d)): fewer key bits = fewer radix passes
  int64_t cell = 128;
  while (ext / cell + 1 >= (1 << 21))
    cell *= 2;
  cellkey_kernel<<<grid_blocks(n, 256), 256, 0, ctx->stream>>>(d_xyz, n, bb[0], bb[1], bb[2], (int)cell, 1, ctx->keys_in.as<uint64_t>(),
                                                               ctx->vals_in.as<int32_t>());
  if (int rc = sort_cells(ctx, n, morton_key_bits(ext, (int)cell), true))
    return rc;
  BS_HIP(ctx, hipGetLastError());
  ctx->order_n = n;
  ctx->order_xyz = d_xyz;
  return BS_OK;
}

// ---- batched grid (bs_segment_batch) ------------------------------------------------------------------------------
// n_tiles clouds, concatenated, in ONE cell-sorted order (bs_common.h, TiledGridDev): per-tile boxes from one segmented
// reduction, keys (tile << mbits) | Morton(cell in the tile's box) at one shared cell edge, the same radix sort and
// run-length encoding as build_grid, and a hash table keyed by the sort key itself.

namespace {

constexpr int TILE_CHUNK = 4096;  // points per block of the segmented bounding-box reduction

struct TileBlock {
  int32_t tile, begin, end;
};

__global__ void tile_bbox_kernel(const int32_t* __restrict__ xyz, const TileBlock* __restrict__ blk,
                                 int32_t* __restrict__ mnmx)
{
  const TileBlock b = blk[blockIdx.x];
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  for (int64_t i = b.begin + (int64_t)threadIdx.x; i < b.end; i += blockDim.x) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const int v = xyz[3 * i + a];
      mn[a] = min(mn[a], v);
      mx[a] = max(mx[a], v);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    for (int o = 32; o > 0; o >>= 1) {
      mn[a] = min(mn[a], __shfl_xor(mn[a], o));
      mx[a] = max(mx[a], __shfl_xor(mx[a], o));
    }
  }
  __shared__ int smn[3][4], smx[3][4];
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      smn[a][wv] = mn[a];
      smx[a][wv] = mx[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    int m0 = smn[a][0], m1 = smx[a][0];
    for (int t = 1; t < (int)(blockDim.x >> 6); t++) {
      m0 = min(m0, smn[a][t]);
      m1 = max(m1, smx[a][t]);
    }
    atomicMin(&mnmx[6 * b.tile + a], m0);
    atomicMax(&mnmx[6 * b.tile + 3 + a], m1);
  }
}

__global__ void tiled_cellkey_kernel(const int32_t* __restrict__ xyz, int64_t n, const int32_t* __restrict__ off,
                                     int32_t n_tiles, const TileDesc* __restrict__ tiles, int cell, int mbits,
                                     uint64_t* __restrict__ keys, int32_t* __restrict__ vals)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t t = tile_of(off, n_tiles, i);
  const TileDesc d = tiles[t];
  const uint32_t cx = (uint32_t)(xyz[3 * i] - d.mn[0]) / (uint32_t)cell;
  const uint32_t cy = (uint32_t)(xyz[3 * i + 1] - d.mn[1]) / (uint32_t)cell;
  const uint32_t cz = (uint32_t)(xyz[3 * i + 2] - d.mn[2]) / (uint32_t)cell;
  keys[i] = ((uint64_t)t << mbits) | morton_cell(cx, cy, cz);
  if (vals)
    vals[i] = (int32_t)i;
}

// bs_shift_tiles_to_origin_dev: every point minus its tile's minimum
__global__ void tile_shift_kernel(int32_t* __restrict__ xyz, int64_t n, const int32_t* __restrict__ off,
                                  int32_t n_tiles, const int32_t* __restrict__ mnmx)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t t = tile_of(off, n_tiles, i);
#pragma unroll
  for (int a = 0; a < 3; a++)
    xyz[3 * i + a] -= mnmx[6 * t + a];
}

}  // namespace

// Per-tile {min x,y,z, max x,y,z} into d_mnmx [n_tiles][6] and the host copy mnmx (synchronises).  d_off: the offsets
// as int32 on the device (unused here, the blocks carry their ranges).
int tile_bbox_dev(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_off, const std::vector<int64_t>& off,
                  int32_t* d_mnmx, std::vector<int32_t>& mnmx)
{
  (void)d_off;
  hipStream_t st = ctx->stream;
  const int32_t nt = (int32_t)off.size() - 1;
  std::vector<TileBlock> blk;
  for (int32_t t = 0; t < nt; t++)
    for (int64_t b = off[t]; b < off[t + 1]; b += TILE_CHUNK)
      blk.push_back({t, (int32_t)b, (int32_t)std::min<int64_t>(off[t + 1], b + TILE_CHUNK)});
  mnmx.assign(6 * (size_t)nt, 0);
  for (int32_t t = 0; t < nt; t++)
    for (int a = 0; a < 3; a++) {
      mnmx[6 * t + a] = INT_MAX;
      mnmx[6 * t + 3 + a] = INT_MIN;
    }
  BS_HIP(ctx, ctx->bt[BT_BLK].reserve(sizeof(TileBlock) * std::max<size_t>(blk.size(), 1)));
  BS_HIP(ctx, hipMemcpyAsync(ctx->bt[BT_BLK].p, blk.data(), sizeof(TileBlock) * blk.size(), hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(d_mnmx, mnmx.data(), sizeof(int32_t) * mnmx.size(), hipMemcpyHostToDevice, st));
  if (!blk.empty())
    tile_bbox_kernel<<<(int)blk.size(), 256, 0, st>>>(d_xyz, ctx->bt[BT_BLK].as<TileBlock>(), d_mnmx);
  BS_HIP(ctx, hipMemcpyAsync(mnmx.data(), d_mnmx, sizeof(int32_t) * mnmx.size(), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  return BS_OK;
}

void launch_tile_shift(bs_ctx* ctx, int32_t* d_xyz, int64_t n, const int32_t* d_off, int32_t n_tiles,
                       const int32_t* d_mnmx)
{
  tile_shift_kernel<<<grid_blocks(n, 256), 256, 0, ctx->stream>>>(d_xyz, n, d_off, n_tiles, d_mnmx);
}

// The batch's grid.  The cell edge follows build_grid's rule over the whole batch (the results do not depend on it,
// only the speed), then doubles until tile bits + Morton bits fit the 63-bit key.  A batch of one tile builds the same
// sorted order as build_grid on that cloud.
int build_grid_tiled(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_off, const std::vector<int64_t>& off,
                     double radius, int k, int cell_hint, TiledGridDev* out)
{
  hipStream_t st = ctx->stream;
  const int32_t nt = (int32_t)off.size() - 1;
  const int64_t n = off[nt];
  if (nt < 1 || n <= 0 || n >= (int64_t)INT_MAX - 64)
    return fail(ctx, BS_ERR_INVALID, "point count out of range");
  if (int rc = order_room(ctx, n))
    return rc;
  BS_HIP(ctx, ctx->bt[BT_MNMX].reserve(sizeof(int32_t) * 6 * nt));
  BS_HIP(ctx, ctx->bt[BT_DESC].reserve(sizeof(TileDesc) * nt));

  // 1. per-tile bounding boxes
  std::vector<int32_t> bb;
  int rc = tile_bbox_dev(ctx, d_xyz, d_off, off, ctx->bt[BT_MNMX].as<int32_t>(), bb);
  if (rc != BS_OK)
    return rc;
  const int32_t LIM = 1 << 23;
  int64_t ext = 1;
  for (int32_t t = 0; t < nt; t++)
    for (int a = 0; a < 3; a++) {
      if (bb[6 * t + a] <= -LIM || bb[6 * t + 3 + a] >= LIM) {
        char msg[256];
        snprintf(msg, sizeof msg, "tile %d: coordinates must satisfy |c| < 2^23 mm (8.4 km): shift every tile to its "
                                  "bounding-box origin first (bs_shift_tiles_to_origin_dev)", t);
        return fail(ctx, BS_ERR_RANGE, msg);
      }
      ext = std::max<int64_t>(ext, (int64_t)bb[6 * t + 3 + a] - bb[6 * t + a] + 1);
    }
  int tbits = 0;
  while (((int64_t)1 << tbits) < nt)
    tbits++;
  auto fits = [&](int64_t c) { return ext / c + 1 < (1 << 21) && tbits + morton_key_bits(ext, (int)c) <= 63; };
  std::vector<TileDesc> desc(nt);
  auto upload_desc = [&](int c) -> hipError_t {
    for (int32_t t = 0; t < nt; t++)
      for (int a = 0; a < 3; a++) {
        desc[t].mn[a] = bb[6 * t + a];
        desc[t].dim[a] = (int32_t)(((int64_t)bb[6 * t + 3 + a] - bb[6 * t + a]) / c + 1);
      }
    return hipMemcpyAsync(ctx->bt[BT_DESC].p, desc.data(), sizeof(TileDesc) * nt, hipMemcpyHostToDevice, st);
  };
  BS_HIP(ctx, upload_desc(1));  // (the keys read only the minima)
  const TileDesc* d_desc = ctx->bt[BT_DESC].as<TileDesc>();

  // 2. cell size (build_grid's rule, counted with the tiled keys; the keys are always Morton keys here)
  auto write_keys = [&](int c, bool values) {
    const int mb = morton_key_bits(ext, c);
    tiled_cellkey_kernel<<<grid_blocks(n, 256), 256, 0, st>>>(d_xyz, n, d_off, nt, d_desc, c, mb, ctx->keys_in.as<uint64_t>(),
                                                              values ? ctx->vals_in.as<int32_t>() : nullptr);
    return tbits + mb;
  };
  int cell = 0, sorted_cell = 0;
  rc = trial_cell(ctx, n, ext, radius, k, cell_hint, grid_reuse_on(), write_keys, fits, &cell, &sorted_cell);
  if (rc != BS_OK)
    return rc;
  while (!fits(cell))
    cell *= 2;
  const int mbits = morton_key_bits(ext, cell);
  BS_HIP(ctx, upload_desc(cell));

  // 3 to 6. keys (tile, Morton cell) unless the last trial wrote and sorted them at this cell size; the table is keyed
  // by the sort key itself (morton = 0: stored as it is); the w of a sorted point is its concatenation index
  const bool sorted = sorted_cell == cell;
  const int end_bit = sorted ? 0 : write_keys(cell, true);
  rc = finish_grid(ctx, d_xyz, nullptr, n, end_bit, sorted, 0, cell, out);
  if (rc != BS_OK)
    return rc;
  for (int a = 0; a < 3; a++) {
    out->mn[a] = desc[0].mn[a];
    out->dim[a] = desc[0].dim[a];
  }
  out->tiles = d_desc;
  out->tile_off = d_off;
  out->n_tiles = nt;
  out->mbits = mbits;
  return BS_OK;
}

}  // namespace bs
