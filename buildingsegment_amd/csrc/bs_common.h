// bs_common.h -- shared declarations of the HIP product library
// (libbuildingsegment_hip.so).  gfx950 only; no CUDA, no dual paths.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/bs_api.h"
#include "bs_groundrule.h"

namespace bs {

// ---- scratch guard (bs_selftest_scratch_guard): a test hook, off by default -------------------------------------
// While a context's guard is set, every FRESH allocation of one of its buffers is `bytes + guard` long, reports
// cap == bytes, has its guard filled with SCRATCH_CANARY (flag bit 0) and its front with the poison byte (bit 1).
// The guard is never smaller than the slack of an unguarded allocation, so whatever stays inside its allocation
// without the guard stays inside it with the guard.  bs_selftest_scratch_check reads the guards back.
struct ScratchGuard {
  int flags = 0;  // BS_SCRATCH_CANARY | BS_SCRATCH_POISON
  unsigned char poison = 0;
};
enum : unsigned char { SCRATCH_CANARY = 0xC5 };
inline size_t scratch_guard_bytes(size_t bytes)
{
  const size_t g = bytes / 8 + 256;
  return g < 4096 ? (size_t)4096 : g;
}
// buffers constructed on this thread so far: bs_create compares the growth over `new bs_ctx` with the member table
// of bs_capi.hip, so that a buffer added to bs_ctx and not listed there fails every bs_create
inline thread_local long long scratch_bufs_born = 0;

// ---- small device buffer that only grows, freed with its owner ------------
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  const ScratchGuard* sg = nullptr;  // the owner's guard switch (set by bs_selftest_scratch_guard), nullptr = none
  size_t guard = 0;                  // guard bytes behind cap of this allocation, 0 = unguarded
  DevBuf() { scratch_bufs_born++; }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes)
  {
    if (bytes <= cap)
      return hipSuccess;
    if (p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
    guard = 0;
    if (sg && sg->flags)
      return reserve_guarded(bytes);
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess)
      cap = want;
    return e;
  }
  // the fills are synchronous: done on the device before this returns, whatever stream the caller launches on
  hipError_t reserve_guarded(size_t bytes)
  {
    const size_t g = scratch_guard_bytes(bytes);
    hipError_t e = hipMalloc(&p, bytes + g);
    if (e != hipSuccess)
      return e;
    cap = bytes;
    guard = g;
    if (sg->flags & 1)
      e = hipMemset((char*)p + bytes, SCRATCH_CANARY, g);
    if (e == hipSuccess && (sg->flags & 2))
      e = hipMemset(p, sg->poison, bytes);
    if (e == hipSuccess)
      e = hipDeviceSynchronize();
    return e;
  }
  void release()
  {
    if (p)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
    guard = 0;
  }
  template <class T>
  T* as() const
  {
    return (T*)p;
  }
};

// page-locked host staging (device-to-host results the host loop reads every round: a pageable
// destination goes through the runtime's bounce buffer in chunks, with the GPU idle in between)
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  const ScratchGuard* sg = nullptr;  // as DevBuf (the canary only: the host writes this memory too)
  size_t guard = 0;
  HostBuf() { scratch_bufs_born++; }
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  hipError_t reserve(size_t bytes)
  {
    if (bytes <= cap)
      return hipSuccess;
    if (p)
      (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    guard = 0;
    const bool guarded = sg && sg->flags;
    size_t want = bytes + (guarded ? scratch_guard_bytes(bytes) : bytes / 8 + 256);
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e != hipSuccess)
      return e;
    cap = guarded ? bytes : want;
    if (guarded) {
      guard = want - bytes;
      if (sg->flags & 1)
        memset((char*)p + bytes, SCRATCH_CANARY, guard);
    }
    return e;
  }
  void release()
  {
    if (p)
      (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    guard = 0;
  }
  template <class T>
  T* as() const
  {
    return (T*)p;
  }
};

// ---- search grid (hashed uniform cells over the cell-sorted cloud) --------
struct CellEntry {  // 16 B: one dwordx4 per probe
  uint64_t key;     // packed cell coords, ~0 = empty slot
  int32_t start;    // first sorted position of the cell
  int32_t end;      // one past the last
};

struct GridDev {
  int32_t mn[3];       // bbox min (mm)
  int32_t dim[3];      // cells per axis (< 2^21)
  int32_t cell;        // cell edge (mm)
  uint32_t hmask;      // table size - 1
  const CellEntry* table;
  const int4* spts;    // cell-sorted points: x, y, z, global index
  const int32_t* slocal;  // cell-sorted local (input-order) index
  int64_t n;
};

// Batched grid (bs_segment_batch): one cell-sorted order over n_tiles concatenated clouds.  Every tile keeps its own
// bounding box and cell dims at the shared cell edge, and a cell's key is (tile << mbits) | Morton(cell): the sort
// orders by (tile, Morton cell), so tile t is exactly the sorted positions [tile_off[t], tile_off[t+1]), and the hash
// table (keyed by that same key) never lets a query of one tile see a cell of another.
struct TileDesc {
  int32_t mn[3];   // the tile's bbox min (mm)
  int32_t dim[3];  // its cells per axis
};

struct TiledGridDev : GridDev {  // (mn / dim of the base: unused, every query takes its tile's)
  const TileDesc* tiles;
  const int32_t* tile_off;  // [n_tiles + 1]: concatenation offsets = sorted-position ranges
  int32_t n_tiles;
  int32_t mbits;            // Morton bits of a cell key inside a tile
};

// scratch of the batch (bs_ctx::bt): offsets as int32, bbox blocks, per-tile bbox, descriptors, plane bases, and the
// renumbered plane records / lists of bs_batch_planes_fetch
enum { BT_OFF, BT_BLK, BT_MNMX, BT_DESC, BT_BASE, BT_RECS, BT_LIST, BT_COUNT };

// tile of concatenation index (or sorted position) i: the last t with off[t] <= i (tiles are never empty)
__host__ __device__ inline int32_t tile_of(const int32_t* off, int32_t n_tiles, int64_t i)
{
  int32_t lo = 0, hi = n_tiles - 1;
  while (lo < hi) {
    const int32_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

__host__ __device__ inline uint64_t spread21(uint64_t v)
{
  v &= 0x1FFFFFull;
  v = (v | (v << 32)) & 0x1F00000000FFFFull;
  v = (v | (v << 16)) & 0x1F0000FF0000FFull;
  v = (v | (v << 8)) & 0x100F00F00F00F00Full;
  v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}

__host__ __device__ inline uint64_t morton_cell(uint32_t cx, uint32_t cy, uint32_t cz)
{
  return spread21(cx) | (spread21(cy) << 1) | (spread21(cz) << 2);
}

// The fused pipeline's position-ordered scratch (bs_ctx::seg_npos): n * K neighbour positions, then the n normals
// in POSITION order (the grower builds its records by position and would otherwise gather 24 B per point by
// original index).
__host__ __device__ inline double* pnorm_of(int32_t* npos, int64_t n, int K)
{
  return reinterpret_cast<double*>(npos + (((int64_t)n * K + 1) & ~(int64_t)1));
}

__host__ __device__ inline uint64_t pack_cell(uint32_t cx, uint32_t cy, uint32_t cz)
{
  return (uint64_t)cx | ((uint64_t)cy << 21) | ((uint64_t)cz << 42);
}

__host__ __device__ inline uint32_t hash_cell(uint64_t k)
{
  k *= 0x9E3779B97F4A7C15ull;
  return (uint32_t)(k >> 32) ^ (uint32_t)k;
}

// Workgroups are dealt round-robin over the 8 XCDs (each with its own L2).  For
// kernels that walk the cell-sorted order, map hardware block b to logical
// block (b % 8) * (nb / 8) + b / 8 (grid padded to a multiple of 8) so that one
// XCD sees one contiguous slice of space and spatial neighbours share its L2
// (speed only; any mapping is correct).
__device__ inline int64_t xcd_logical_block()
{
  const int64_t b = blockIdx.x, per = gridDim.x >> 3;
  return (b & 7) * per + (b >> 3);
}
inline int xcd_grid(int64_t nblocks) { return (int)((nblocks + 7) & ~(int64_t)7); }

// ---- plane record produced by region growing ------------------------------
struct PlaneRec {
  double normal[3];
  int64_t list_off;   // offset of pointIdx in the list pool
  int64_t list_n;     // pointIdx.size()
  int32_t center[3];
  int32_t id;         // 1-based plane id
  int32_t seed;
  int32_t pad;
};

struct GrowStats {
  int32_t n_planes;
  int32_t error;        // != 0: pool overflow / watchdog
  int64_t list_used;
  int64_t seed_attempts;
  int64_t largest;
  int64_t steps;
};

}  // namespace bs

// ---- context ---------------------------------------------------------------
// the streams and events of a context: a base, so that they go after every buffer of bs_ctx has freed itself
struct bs_ctx_handles {
  hipStream_t own_stream = nullptr;
  hipEvent_t ev[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t side = nullptr;  // second stream of the grower (validate3 beside the owner passes)
  hipEvent_t sev[2] = {nullptr, nullptr};
  ~bs_ctx_handles()
  {
    for (auto& e : ev)
      if (e)
        (void)hipEventDestroy(e);
    for (auto& e : sev)
      if (e)
        (void)hipEventDestroy(e);
    if (side)
      (void)hipStreamDestroy(side);
    if (own_stream)
      (void)hipStreamDestroy(own_stream);
  }
};

struct bs_ctx : bs_ctx_handles {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bs_timings tm{};
  bs::ScratchGuard sg;  // bs_selftest_scratch_guard (off)

  // grid scratch
  bs::DevBuf keys_in, keys_out, vals_in, vals_out, cub_tmp, uniq_keys, uniq_cnt, misc;
  bs::DevBuf table, spts;
  // kNN scratch
  bs::DevBuf fb_list, d_xyz_h, d_neigh_h, d_normals_h, d_plane_h;
  // pipeline scratch (bs_segment_dev with NULL outputs)
  bs::DevBuf seg_neigh, seg_normals;
  // region-grow state
  bs::DevBuf rg_list, rg_stack, rg_planes, rg_stats, rg_aux, rg_pstore, rg_rec, rg_radj, rg_roff, rg_geo, rg_gs, rg_disp;
  bs::HostBuf rg_hout;  // PlaneOut[wave_cap + MAX_PENDING] + a few scalars, page-locked
  int64_t rg_n = 0;
  bool rg_valid = false;
  // final owner structure of the last speculative grow (inside rg_aux): owner by POSITION and the original index
  // of every position -- what bs_owner_fetch_dev maps back to the caller's order
  const int32_t* rg_omega = nullptr;
  const int32_t* rg_prio = nullptr;
  const int32_t* rg_seeds = nullptr;  // committed seeds (original indices, ascending = commit order), device
  int32_t rg_nplanes = 0;
  int forge_mode = 0;  // bs_selftest_forge_next
  int audit = 0;       // bs_set_audit
  bs_grow_limits lim{0, 0, 0, 0, -1, -1, 0, 0};  // bs_selftest_grow_limits (all defaults)
  bs_grow_counters gc{};                         // bs_get_grow_counters
  // 2-D raster scratch (bs_raster.hip)
  bs::DevBuf rs_keys_in, rs_keys_out, rs_vals_in, rs_vals_out, rs_cnt, rs_img, rs_tmp;
  // cell-sorted order of the last grid build (vals_out): spatially coherent iteration for gathers
  int64_t order_n = 0;
  const int32_t* order_xyz = nullptr;
  // neighbour rows as cell-sorted POSITIONS (rows in position order), written by the kNN kernels of the fused
  // pipeline for the same cloud / k / neigh buffer: the grower takes them instead of translating indices
  bs::DevBuf seg_npos;
  // scratch of the sharded pass (bs_sharded.hip): named by use there
  bs::DevBuf fp[23];  // scratch of bs_footprints[_dev] (bs_contour.hip)
  bs::DevBuf bd[14];  // scratch of the building map, assignment and votes (bs_building.hip)
  bs::DevBuf rf[15];  // scratch of the roof stage (bs_roof.hip)
  bs::DevBuf ft[5];   // scratch of the plane fit (bs_fit.hip)
  // solids (bs_solid.hip): scratch, and what bs_solids_count_dev leaves for bs_solids_emit_dev (tops, clean map, offsets)
  bs::DevBuf sd[14];
  bool sd_valid = false;
  int32_t sd_w = 0, sd_h = 0, sd_bin = 0, sd_base = 0;
  bool sd_bases = false;  // the count ran under bs_set_building_bases: the emit reads bases_dev
  int64_t sd_nv = 0, sd_nf = 0, sd_ni = 0;
  double sd_ms_emit[2] = {0, 0};  // vertex pass, face pass of the last emit
  bs::DevBuf fc[16];  // scratch of the roof facets and their edges (bs_facet.hip)
  // facet outlines (bs_outline.hip): scratch, and what bs_facet_outlines_count_dev leaves for bs_facet_outlines_emit_dev
  // (per half-edge: its number, its place in the vertex arrays or -1, its Z)
  bs::DevBuf ol[27];
  bool ol_valid = false, ol_has_z = false;
  int32_t ol_w = 0, ol_nr = 0;      // (ol_nr, ol_leader: the ring count and the leader of every half-edge, for bs_simplify.hip)
  const int32_t* ol_leader = nullptr;
  int64_t ol_nhalf = 0, ol_nv = 0;
  double ol_ms_emit = 0;  // the last emit
  // simplified outlines (bs_simplify.hip): scratch, and what bs_simple_outlines_count_dev leaves for
  // bs_simple_outlines_emit_dev (the finished vertex arrays)
  bs::DevBuf sp[39];
  bool sp_valid = false, sp_has_z = false;
  int64_t sp_nsv = 0;
  double sp_ms_emit = 0;  // the last emit
  // what the last successful bs_simple_outlines_count_dev leaves for the clean outlines (bs_uncross.hip): the node arrays
  // in the rotated order, the kept flags (seg[cur].x == -1), the round buffers and the ring figures, all inside sp
  struct SimplifyState {
    int32_t N = 0, nr = 0, cur = 0;
    int2* seg[2] = {nullptr, nullptr};
    unsigned long long* best[2] = {nullptr, nullptr};
    unsigned long long* tie[2] = {nullptr, nullptr};
    unsigned long long* c2 = nullptr;
    uint8_t* forced = nullptr;
    const int2* xy = nullptr;
    const int32_t *cidx = nullptr, *z = nullptr, *right = nullptr, *ring = nullptr, *noff = nullptr, *rot = nullptr;
    const uint8_t* flag = nullptr;
  } sp_state;
  // clean outlines (bs_uncross.hip): scratch, and what bs_clean_outlines_count_dev leaves for bs_clean_outlines_emit_dev
  bs::DevBuf uc[29];
  bool uc_valid = false, uc_has_z = false;
  int64_t uc_nsv = 0;
  double uc_ms_emit = 0;
  // sweeps (bs_sweep.hip): the mode of bs_set_outline_sweeps, the figures of the last successful clean count, scratch
  int sweeps_mode = 0;
  bs_outline_sweeps sweeps{};
  bs::DevBuf sw[8];
  // what the last successful bs_clean_outlines_count_dev leaves for the outline triangles (bs_triangulate.hip), all inside
  // uc: the clean vertices, the ring of every vertex, the first vertex of every ring
  const int2* uc_xy = nullptr;
  const int32_t *uc_ring = nullptr, *uc_soff = nullptr;
  const int32_t *uc_z = nullptr, *uc_right = nullptr;  // (their Z and right labels, for bs_polysolid.hip)
  // outline triangles (bs_triangulate.hip): scratch, and what bs_outline_triangles_count_dev leaves for
  // bs_outline_triangles_emit_dev (the triangles)
  bs::DevBuf tr[13];
  bool tr_valid = false;
  int64_t tr_ntri = 0;
  double tr_ms_emit = 0;
  const int32_t* tr_tri = nullptr;  // (the triangles of the last count, inside tr, for bs_polysolid.hip)
  // (for bs_modelraster.hip: tri_offset [tr_nl + 1] of the last count on the device, inside tr, nullptr without a ring; the
  // label count and the image size of that count)
  const long long* tr_toff = nullptr;
  int32_t tr_nl = 0, tr_w = 0, tr_h = 0;
  // polygon solids (bs_polysolid.hip): scratch, and what bs_poly_solids_count_dev leaves for bs_poly_solids_emit_dev (the
  // twins, the vertex numbers, the offsets); the emit also reads the clean vertices and the triangles, so a later clean
  // count on this context ends its validity
  bs::DevBuf ps[29];
  bool ps_valid = false;
  int32_t ps_bin = 0, ps_base = 0, ps_nl = 0, ps_nr = 0, ps_nsv = 0;
  bool ps_bases = false;  // the count ran under bs_set_building_bases: the emit reads bases_dev
  int64_t ps_nv = 0, ps_nf = 0, ps_ni = 0, ps_ntri = 0;
  double ps_ms_emit[2] = {0, 0};  // vertex pass, face passes of the last emit
  bs::DevBuf mr[13];  // scratch of the model raster (bs_modelraster.hip); it keeps no state between calls
  bs::DevBuf pr[15];  // scratch of the point residuals (bs_pointresid.hip); it keeps no state between calls
  bs::DevBuf gn[32];  // scratch of the roof generalisation (bs_generalise.hip); it keeps no state between calls
  // per-building bases (bs_set_building_bases): the host table, its copy on the device; empty = off
  std::vector<int32_t> bases;
  bs::DevBuf bases_dev;
  bs::DevBuf tn[15];  // scratch of the terrain stage (bs_terrain.hip); it keeps no state between calls
  bs::DevBuf gd[10];  // scratch of the ground stage (bs_ground.hip); it keeps no state between calls
  // ground model (bs_set_ground_model): the device copy of the table and its lattice; gm_on == false = off
  bs::DevBuf gm_dev;
  bool gm_on = false;
  int32_t gm_w = 0, gm_h = 0, gm_cell = 0, gm_min = 0;
  bs::DevBuf evd[10];  // scratch of the roof evidence (bs_evidence.hip); it keeps no state between calls
  // oriented boxes (bs_hull.hip): scratch, and what bs_label_hulls_count_dev leaves for bs_label_hulls_emit_dev (the strict
  // hull vertices in their final order)
  bs::DevBuf hl[25];
  bool hl_valid = false;
  int64_t hl_nv = 0;
  const int32_t* hl_xy = nullptr;  // (inside hl)
  double hl_ms_emit = 0;           // the last emit
  // footprint screen (bs_set_footprint_screen): the image bs_footprints ANDs into its mask; fs_ptr == nullptr = off.  The host
  // form keeps a copy in fs_dev, the _dev form the caller's pointer
  bs::DevBuf fs_dev;
  const uint8_t* fs_ptr = nullptr;
  int32_t fs_w = 0, fs_h = 0;
  bs::DevBuf sh[25];  // (24 scratch buffers of bs_sharded.hip + the look-up table of bs_remap_rows_dev)
  std::vector<int32_t> sh_seeds;  // all committed seeds of the last bs_segment_sharded (global indices, ascending)
  int64_t sh_nloc = 0;            // points this rank grew
  bool sh_valid = false;
  const int32_t* npos_neigh = nullptr;
  const double* npos_normals = nullptr;
  int npos_k = 0;
  // bs_segment_batch: scratch, and the tiling of the last batch (valid while its region-grow result is)
  bs::DevBuf bt[bs::BT_COUNT];
  std::vector<int64_t> bt_off;
  bool bt_valid = false;
  // per-tile descriptors of bs_grid_picture_batch_dev / bs_footprints_batch_dev (uploaded by each call)
  bs::DevBuf tile_desc;
};

namespace bs {

int fail(bs_ctx* ctx, int status, const char* what, hipError_t e = hipSuccess);

#define BS_HIP(ctx, call)                                     \
  do {                                                        \
    hipError_t _e = (call);                                   \
    if (_e != hipSuccess)                                     \
      return bs::fail((ctx), BS_ERR_HIP, #call, _e);          \
  } while (0)

// simplify.hip: one Douglas-Peucker round in which every segment whose left end `forced` marks splits at its choice
// whatever the tolerance (bs_uncross.hip activates only the nodes of marked segments, and marks all of those)
void simplify_forced_round(hipStream_t st, int32_t N, const int2* seg, const int2* xy, const int32_t* cidx,
                           unsigned long long* c2, unsigned long long* best, unsigned long long* tie, const uint8_t* forced,
                           int2* seg2, unsigned long long* best2, unsigned long long* tie2, int* changed, int* err);
// grid.hip
int build_grid(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_gidx, int64_t n, double radius,
               int k, int cell_hint, GridDev* out);
int build_spatial_order(bs_ctx* ctx, const int32_t* d_xyz, int64_t n);
int bbox_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bb[6]);
// batched grid (bs_batch.hip names the scratch): tile_off_dev = the offsets as int32 on the device
int tile_bbox_dev(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_off, const std::vector<int64_t>& off,
                  int32_t* d_mnmx, std::vector<int32_t>& mnmx);
int build_grid_tiled(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_off, const std::vector<int64_t>& off,
                     double radius, int k, int cell_hint, TiledGridDev* out);
// batch.hip: tile_offset checks of every batch entry point (errors name the tile); *total = tile_offset[n_tiles]
int check_tiles(bs_ctx* ctx, const int64_t* off, int32_t n_tiles, int64_t min_pts, int64_t* total);
void launch_tile_shift(bs_ctx* ctx, int32_t* d_xyz, int64_t n, const int32_t* d_off, int32_t n_tiles,
                       const int32_t* d_mnmx);
// knn.hip
int launch_knn_normals(bs_ctx* ctx, const GridDev& g, int64_t q_begin, int64_t q_end,
                       const bs_params& p, int32_t* d_neigh, double* d_normals, double cert_radius,
                       int64_t* n_uncertified, int32_t* d_npos = nullptr);
int launch_knn_normals_tiled(bs_ctx* ctx, const TiledGridDev& g, const bs_params& p, int32_t* d_neigh,
                             double* d_normals, int32_t* d_npos);
// capi.hip: the device table of bs_set_building_bases for a call over n_buildings, nullptr while the switch is off;
// BS_ERR_INVALID (worded for `who`) where the table's length differs
int building_bases(bs_ctx* ctx, int32_t n_buildings, const char* who, const int32_t** d_table);
// capi.hip: the rule of bs_set_ground_model for a kernel (table == nullptr while the switch is off)
GroundRule ground_rule(const bs_ctx* ctx);
int region_grow_dev_impl(bs_ctx* ctx, const int32_t* d_xyz, const double* d_normals, const int32_t* d_neigh,
                         int64_t n, const bs_params* p, int32_t* d_plane_idx, bool trusted_neigh);
int check_params(bs_ctx* ctx, const bs_params* p, int64_t n);
int planes_to_host(bs_ctx* ctx, const PlaneRec* d_recs, const int32_t* d_list, int np, int64_t list_used,
                   bs_planes* out);
// grow.hip
int launch_region_grow_seq(bs_ctx* ctx, const int32_t* d_xyz, const double* d_normals,
                           const int32_t* d_neigh, int64_t n, const bs_params& p,
                           int32_t* d_plane_idx);
// grow_spec.hip
int launch_region_grow_spec(bs_ctx* ctx, const int32_t* d_xyz, const double* d_normals,
                            const int32_t* d_neigh, int64_t n, const bs_params& p,
                            int32_t* d_plane_idx);

}  // namespace bs
