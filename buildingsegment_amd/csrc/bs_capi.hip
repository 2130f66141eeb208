// bs_capi.hip -- extern "C" boundary of libbuildingsegment_hip.so
// (declarations and reference citations: include/bs_api.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "bs_host.h"

namespace bs {

int fail(bs_ctx* ctx, int status, const char* what, hipError_t e)
{
  if (ctx) {
    ctx->err = what ? what : "";
    if (e != hipSuccess) {
      ctx->err += ": ";
      ctx->err += hipGetErrorString(e);
    }
  }
  return status;
}

int building_bases(bs_ctx* ctx, int32_t n_buildings, const char* who, const int32_t** d_table)
{
  *d_table = nullptr;
  if (ctx->bases.empty())
    return BS_OK;
  if ((size_t)n_buildings != ctx->bases.size()) {
    const std::string msg = std::string(who) + ": n_buildings differs from the table of bs_set_building_bases";
    return fail(ctx, BS_ERR_INVALID, msg.c_str());
  }
  *d_table = ctx->bases_dev.as<int32_t>();
  return BS_OK;
}

GroundRule ground_rule(const bs_ctx* ctx)
{
  if (!ctx->gm_on)
    return GroundRule{nullptr, 0, 0, 1, 0};
  return GroundRule{ctx->gm_dev.as<int32_t>(), ctx->gm_w, ctx->gm_h, ctx->gm_cell, ctx->gm_min};
}

int check_params(bs_ctx* ctx, const bs_params* p, int64_t n)
{
  if (!p)
    return fail(ctx, BS_ERR_INVALID, "params is NULL");
  if (p->k < 2 || p->k > 32)
    return fail(ctx, BS_ERR_INVALID, "k must be in [2, 32]");
  if (p->max_nn < 3 || p->max_nn > 64)
    return fail(ctx, BS_ERR_INVALID, "max_nn must be in [3, 64]");
  if (!(p->radius > 0.0) || p->radius > 1.0e6)
    return fail(ctx, BS_ERR_INVALID, "radius must be in (0, 1e6]");
  if (p->th_thickness < 0 || p->th_point_count < 0)
    return fail(ctx, BS_ERR_INVALID, "thresholds must be >= 0");
  if (n < p->k)
    return fail(ctx, BS_ERR_INVALID, "n < k (the reference is undefined there)");
  if (n >= (int64_t)INT32_MAX - 64)
    return fail(ctx, BS_ERR_INVALID, "n must fit in int32");
  if (p->rg_mode < 0 || p->rg_mode > 2)
    return fail(ctx, BS_ERR_INVALID, "rg_mode must be 0, 1 or 2");
  return BS_OK;
}

struct EventTimer {
  bs_ctx* ctx;
  explicit EventTimer(bs_ctx* c) : ctx(c) {}
  void mark(int i) { (void)hipEventRecord(ctx->ev[i], ctx->stream); }
  double ms(int i, int j)
  {
    float t = 0.f;
    if (hipEventElapsedTime(&t, ctx->ev[i], ctx->ev[j]) != hipSuccess)
      return 0.0;
    return (double)t;
  }
};

// foreign neighbour arrays are dereferenced on the device: one streaming pass proves them in range
__global__ void neigh_range_kernel(const int32_t* __restrict__ neigh, int64_t total, int32_t n, int* bad)
{
  bool b = false;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = neigh[i];
    b = b || v < 0 || v >= n;
  }
  if (__syncthreads_or(b) && threadIdx.x == 0)
    *bad = 1;
}

int region_grow_dev_impl(bs_ctx* ctx, const int32_t* d_xyz, const double* d_normals, const int32_t* d_neigh,
                         int64_t n, const bs_params* p, int32_t* d_plane_idx, bool trusted_neigh)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_xyz || !d_normals || !d_neigh || !d_plane_idx)
    return fail(ctx, BS_ERR_INVALID, "null device pointer");
  int rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  if (!trusted_neigh) {
    BS_HIP(ctx, ctx->misc.reserve(256));
    int* d_bad = ctx->misc.as<int>() + 48;
    BS_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(int), ctx->stream));
    const int64_t total = n * (int64_t)p->k;
    neigh_range_kernel<<<(int)std::min<int64_t>((total + 255) / 256, 65536), 256, 0, ctx->stream>>>(d_neigh, total, (int32_t)n, d_bad);
    int bad = 0;
    BS_HIP(ctx, hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad)
      return fail(ctx, BS_ERR_INVALID, "neighbour index out of range");
  }
  EventTimer T(ctx);
  T.mark(3);
  if (p->rg_mode == 1)
    rc = launch_region_grow_seq(ctx, d_xyz, d_normals, d_neigh, n, *p, d_plane_idx);
  else
    rc = launch_region_grow_spec(ctx, d_xyz, d_normals, d_neigh, n, *p, d_plane_idx);
  if (rc != BS_OK)
    return rc;
  T.mark(4);
  BS_HIP(ctx, hipEventSynchronize(ctx->ev[4]));
  ctx->tm.grow_ms = T.ms(3, 4);
  return BS_OK;
}

// np device plane records + their list pool -> a host bs_planes (what bs_planes_fetch and bs_batch_planes_fetch return)
int planes_to_host(bs_ctx* ctx, const PlaneRec* d_recs, const int32_t* d_list, int np, int64_t list_used,
                   bs_planes* out)
{
  out->n_planes = np;
  out->id = (int32_t*)malloc(sizeof(int32_t) * std::max(np, 1));
  out->normal = (double*)malloc(sizeof(double) * 3 * std::max(np, 1));
  out->center = (int32_t*)malloc(sizeof(int32_t) * 3 * std::max(np, 1));
  out->offset = (int64_t*)malloc(sizeof(int64_t) * (np + 1));
  out->point_idx = (int32_t*)malloc(sizeof(int32_t) * std::max<int64_t>(list_used, 1));
  PlaneRec* recs = (PlaneRec*)malloc(sizeof(PlaneRec) * std::max(np, 1));
  if (!out->id || !out->normal || !out->center || !out->offset || !out->point_idx || !recs) {
    free(recs);
    bs_planes_free(out);
    return fail(ctx, BS_ERR_NOMEM, "host allocation failed");
  }
  hipError_t he = hipSuccess;
  if (np > 0)
    he = hipMemcpy(recs, d_recs, sizeof(PlaneRec) * np, hipMemcpyDeviceToHost);
  if (he == hipSuccess && list_used > 0)
    he = hipMemcpy(out->point_idx, d_list, sizeof(int32_t) * list_used, hipMemcpyDeviceToHost);
  if (he != hipSuccess) {
    free(recs);
    bs_planes_free(out);
    return fail(ctx, BS_ERR_HIP, "bs_planes_fetch: copy of the plane records failed", he);
  }
  for (int i = 0; i < np; i++) {
    out->id[i] = recs[i].id;
    for (int a = 0; a < 3; a++) {
      out->normal[3 * i + a] = recs[i].normal[a];
      out->center[3 * i + a] = recs[i].center[a];
    }
    out->offset[i] = recs[i].list_off;
  }
  out->offset[np] = list_used;
  free(recs);
  return BS_OK;
}

}  // namespace bs

using namespace bs;

namespace {
bool scratch_members_complete(bs_ctx* c, long long born, int64_t* n_members);  // (with the scratch guard, below)
}

extern "C" {

int bs_api_version(void) { return BS_API_VERSION; }

int64_t bs_sizeof_timings(void) { return (int64_t)sizeof(bs_timings); }

const char* bs_strerror(int status)
{
  switch (status) {
  case BS_OK: return "ok";
  case BS_ERR_INVALID: return "invalid argument";
  case BS_ERR_RANGE: return "coordinate outside the exact domain (|c| < 2^23 mm): shift the cloud to its bounding-box origin first (bs_shift_to_origin_dev / the buildingSeg constructor)";
  case BS_ERR_NOMEM: return "out of memory";
  case BS_ERR_HIP: return "HIP runtime error";
  case BS_ERR_NO_DEVICE: return "no usable HIP device";
  case BS_ERR_INTERNAL: return "internal invariant violated";
  case BS_ERR_UNCERTIFIED: return "halo too thin to certify every k-list";
  default: return "unknown status";
  }
}

void bs_params_default(bs_params* p)
{
  if (!p)
    return;
  p->k = 15;              // TMC3.cpp:215-216
  p->max_nn = 50;         // my_function.h:63
  p->radius = 100.0;      // my_function.h:63
  p->th_thickness = 300;  // my_function.h:117
  p->th_point_count = 400;  // my_function.h:118
  p->cos_th = 0.88;       // my_function.cpp:230
  p->cell_size = 0;
  p->rg_mode = 0;
}

int bs_create(int device, bs_ctx** out)
{
  if (!out)
    return BS_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return BS_ERR_NO_DEVICE;
  if (device < 0 || device >= count)
    return BS_ERR_INVALID;
  if (hipSetDevice(device) != hipSuccess)
    return BS_ERR_NO_DEVICE;
  const long long born = scratch_bufs_born;
  bs_ctx* c = new (std::nothrow) bs_ctx();
  if (!c)
    return BS_ERR_NOMEM;
  if (!scratch_members_complete(c, scratch_bufs_born - born, nullptr)) {  // a buffer of bs_ctx the member table omits
    delete c;
    return BS_ERR_INTERNAL;
  }
  c->device = device;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return BS_ERR_HIP;
  }
  c->stream = c->own_stream;
  for (auto& e : c->ev)
    if (hipEventCreate(&e) != hipSuccess) {
      bs_destroy(c);
      return BS_ERR_HIP;
    }
  *out = c;
  return BS_OK;
}

void bs_destroy(bs_ctx* c)
{
  if (!c)
    return;
  (void)hipSetDevice(c->device);
  if (c->stream)
    (void)hipStreamSynchronize(c->stream);
  delete c;  // the buffers free themselves, then the events and the streams go (bs_ctx_handles)
}

const char* bs_last_error(const bs_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int bs_set_stream(bs_ctx* ctx, void* hip_stream)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return BS_OK;
}

int bs_get_timings(const bs_ctx* ctx, bs_timings* out)
{
  if (!ctx || !out)
    return BS_ERR_INVALID;
  *out = ctx->tm;
  return BS_OK;
}

// ---------------------------------------------------------------------------
// device-buffer entry points
// ---------------------------------------------------------------------------

static int knn_normals_dev_impl(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_gidx, int64_t n, int64_t q_begin,
                                int64_t q_end, const bs_params* p, int32_t* d_neigh, double* d_normals,
                                double cert_radius, int64_t* n_uncertified, int32_t* d_npos)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_xyz || !d_neigh)
    return fail(ctx, BS_ERR_INVALID, "null device pointer");
  int rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  if (q_begin < 0 || q_end > n || q_begin > q_end)
    return fail(ctx, BS_ERR_INVALID, "bad query range");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  EventTimer T(ctx);
  T.mark(0);
  GridDev g;
  rc = build_grid(ctx, d_xyz, d_gidx, n, p->radius, p->k, p->cell_size, &g);
  if (rc != BS_OK)
    return rc;
  T.mark(1);
  ctx->npos_neigh = nullptr;
  ctx->npos_normals = nullptr;
  rc = launch_knn_normals(ctx, g, q_begin, q_end, *p, d_neigh, d_normals, cert_radius, n_uncertified, d_npos);
  if (rc != BS_OK)
    return rc;
  T.mark(2);
  BS_HIP(ctx, hipEventSynchronize(ctx->ev[2]));
  ctx->tm.grid_ms = T.ms(0, 1);
  ctx->tm.knn_ms = T.ms(1, 2);
  ctx->tm.total_ms = T.ms(0, 2);
  if (d_npos) {  // valid for exactly this neighbour buffer / k (checked by the grower)
    ctx->npos_neigh = d_neigh;
    ctx->npos_normals = d_normals;
    ctx->npos_k = p->k;
  }
  return BS_OK;
}

int bs_knn_normals_dev(bs_ctx* ctx, const int32_t* d_xyz, const int32_t* d_gidx, int64_t n, int64_t q_begin,
                       int64_t q_end, const bs_params* p, int32_t* d_neigh, double* d_normals,
                       double cert_radius, int64_t* n_uncertified)
{
  return knn_normals_dev_impl(ctx, d_xyz, d_gidx, n, q_begin, q_end, p, d_neigh, d_normals, cert_radius, n_uncertified,
                              nullptr);
}

int bs_region_grow_dev(bs_ctx* ctx, const int32_t* d_xyz, const double* d_normals, const int32_t* d_neigh,
                       int64_t n, const bs_params* p, int32_t* d_plane_idx)
{
  if (ctx) {  // the position-ordered copies of the fused pipeline are keyed by pointer, and these buffers' CONTENTS may
    ctx->npos_neigh = nullptr;  // have changed since: only bs_segment[_dev] itself hands them on to the grower
    ctx->npos_normals = nullptr;
  }
  return region_grow_dev_impl(ctx, d_xyz, d_normals, d_neigh, n, p, d_plane_idx, false);
}

int bs_segment_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const bs_params* p, int32_t* d_neigh,
                   double* d_normals, int32_t* d_plane_idx)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_xyz || !d_plane_idx)
    return fail(ctx, BS_ERR_INVALID, "null device pointer");
  int rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  if (!d_neigh) {
    BS_HIP(ctx, ctx->seg_neigh.reserve(sizeof(int32_t) * n * p->k));
    d_neigh = ctx->seg_neigh.as<int32_t>();
  }
  if (!d_normals) {
    BS_HIP(ctx, ctx->seg_normals.reserve(sizeof(double) * n * 3));
    d_normals = ctx->seg_normals.as<double>();
  }
  EventTimer T(ctx);
  T.mark(5);
  // the fused pipeline also keeps every neighbour's cell-sorted position for the grower (speculative mode)
  int32_t* d_npos = nullptr;
  if (p->rg_mode != 1) {
    BS_HIP(ctx, ctx->seg_npos.reserve(sizeof(int32_t) * ((size_t)n * p->k + 2) + sizeof(double) * 3 * (size_t)n));  // + normals by position
    d_npos = ctx->seg_npos.as<int32_t>();
  }
  rc = knn_normals_dev_impl(ctx, d_xyz, nullptr, n, 0, n, p, d_neigh, d_normals, 0.0, nullptr, d_npos);
  if (rc != BS_OK)
    return rc;
  rc = region_grow_dev_impl(ctx, d_xyz, d_normals, d_neigh, n, p, d_plane_idx, true);  // our own k-lists: in range
  if (rc != BS_OK)
    return rc;
  ctx->tm.total_ms = T.ms(5, 4);
  return BS_OK;
}

int bs_selftest_forge_next(bs_ctx* ctx, int mode)
{
  if (!ctx || mode < 0 || mode > 2)
    return BS_ERR_INVALID;
  ctx->forge_mode = mode;
  return BS_OK;
}

int bs_set_outline_sweeps(bs_ctx* ctx, int32_t mode)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (mode < 0 || mode > 2)
    return bs::fail(ctx, BS_ERR_INVALID, "outline sweeps: the mode is 0 (off), 1 (report) or 2 (repair)");
  ctx->sweeps_mode = mode;
  return BS_OK;
}

int bs_get_outline_sweeps(bs_ctx* ctx, struct bs_outline_sweeps* out)
{
  if (!ctx || !out)
    return BS_ERR_INVALID;
  *out = ctx->sweeps;
  if (out->wave_cap == 0) {  // (no clean count yet)
    out->mode = ctx->sweeps_mode;
    out->wave_cap = BS_SWEEP_WAVE_CAP;
  }
  return BS_OK;
}

int bs_set_building_bases(bs_ctx* ctx, const int32_t* base, int32_t n_buildings)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (n_buildings < 0 || (n_buildings > 0 && !base))
    return bs::fail(ctx, BS_ERR_INVALID, "building bases: a null table with n_buildings > 0, or n_buildings < 0");
  // a count under another table (or none) must not be emitted under this one
  ctx->sd_valid = false;
  ctx->ps_valid = false;
  ctx->bases.clear();  // (off, also where the copy below fails)
  if (!base || n_buildings == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  BS_HIP(ctx, ctx->bases_dev.reserve(4 * (size_t)n_buildings));
  BS_HIP(ctx, hipMemcpyAsync(ctx->bases_dev.p, base, 4 * (size_t)n_buildings, hipMemcpyHostToDevice, ctx->stream));
  BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->bases.assign(base, base + n_buildings);
  return BS_OK;
}

int bs_get_building_bases(bs_ctx* ctx, int32_t* base, int32_t capacity, int32_t* n_buildings)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!n_buildings || capacity < 0 || (capacity > 0 && !base))
    return bs::fail(ctx, BS_ERR_INVALID, "building bases: a null pointer or a negative capacity");
  *n_buildings = (int32_t)ctx->bases.size();
  const size_t m = std::min<size_t>((size_t)capacity, ctx->bases.size());
  if (m)
    memcpy(base, ctx->bases.data(), 4 * m);
  return BS_OK;
}

static int set_ground_model(bs_ctx* ctx, const int32_t* dtm, bool on_device, int32_t width, int32_t height, int32_t cell,
                            int32_t min_height)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!dtm) {
    ctx->gm_on = false;
    return BS_OK;
  }
  if (width < 1 || height < 1 || cell < 1 || min_height < 0 || (long long)width * height >= (1ll << 31) - 1)
    return bs::fail(ctx, BS_ERR_INVALID, "ground model: width, height or cell < 1, width * height >= 2^31 - 1, or min_height < 0");
  ctx->gm_on = false;  // (off, also where the copy below fails)
  const size_t bytes = 4 * (size_t)width * (size_t)height;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  BS_HIP(ctx, ctx->gm_dev.reserve(bytes));
  BS_HIP(ctx, hipMemcpyAsync(ctx->gm_dev.p, dtm, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->gm_w = width;
  ctx->gm_h = height;
  ctx->gm_cell = cell;
  ctx->gm_min = min_height;
  ctx->gm_on = true;
  return BS_OK;
}

int bs_set_ground_model(bs_ctx* ctx, const int32_t* dtm, int32_t width, int32_t height, int32_t cell, int32_t min_height)
{
  return set_ground_model(ctx, dtm, false, width, height, cell, min_height);
}

int bs_set_ground_model_dev(bs_ctx* ctx, const int32_t* d_dtm, int32_t width, int32_t height, int32_t cell, int32_t min_height)
{
  return set_ground_model(ctx, d_dtm, true, width, height, cell, min_height);
}

int bs_get_ground_model(bs_ctx* ctx, int32_t* dtm, int64_t capacity, int32_t* width, int32_t* height, int32_t* cell,
                        int32_t* min_height)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!width || !height || !cell || !min_height || capacity < 0 || (capacity > 0 && !dtm))
    return bs::fail(ctx, BS_ERR_INVALID, "ground model: a null pointer or a negative capacity");
  *width = ctx->gm_on ? ctx->gm_w : 0;
  *height = ctx->gm_on ? ctx->gm_h : 0;
  *cell = ctx->gm_on ? ctx->gm_cell : 0;
  *min_height = ctx->gm_on ? ctx->gm_min : 0;
  const int64_t m = ctx->gm_on ? std::min<int64_t>(capacity, (int64_t)ctx->gm_w * ctx->gm_h) : 0;
  if (m > 0) {
    BS_HIP(ctx, hipSetDevice(ctx->device));
    BS_HIP(ctx, hipMemcpyAsync(dtm, ctx->gm_dev.p, 4 * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return BS_OK;
}

static int set_footprint_screen(bs_ctx* ctx, const uint8_t* keep, bool on_device, int32_t width, int32_t height)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!keep) {
    ctx->fs_ptr = nullptr;
    return BS_OK;
  }
  if (width < 1 || height < 1 || (long long)width * height >= (1ll << 31) - 1)
    return bs::fail(ctx, BS_ERR_INVALID, "footprint screen: width or height < 1, or width * height >= 2^31 - 1");
  ctx->fs_ptr = nullptr;  // (off, also where the copy below fails)
  if (!on_device) {
    const size_t bytes = (size_t)width * (size_t)height;
    BS_HIP(ctx, hipSetDevice(ctx->device));
    BS_HIP(ctx, ctx->fs_dev.reserve(bytes));
    BS_HIP(ctx, hipMemcpyAsync(ctx->fs_dev.p, keep, bytes, hipMemcpyHostToDevice, ctx->stream));
    BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    keep = ctx->fs_dev.as<uint8_t>();
  }
  ctx->fs_w = width;
  ctx->fs_h = height;
  ctx->fs_ptr = keep;
  return BS_OK;
}

int bs_set_footprint_screen(bs_ctx* ctx, const uint8_t* keep, int32_t width, int32_t height)
{
  return set_footprint_screen(ctx, keep, false, width, height);
}

int bs_set_footprint_screen_dev(bs_ctx* ctx, const uint8_t* d_keep, int32_t width, int32_t height)
{
  return set_footprint_screen(ctx, d_keep, true, width, height);
}

int bs_get_footprint_screen(bs_ctx* ctx, uint8_t* keep, int64_t capacity, int32_t* width, int32_t* height)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!width || !height || capacity < 0 || (capacity > 0 && !keep))
    return bs::fail(ctx, BS_ERR_INVALID, "footprint screen: a null pointer or a negative capacity");
  *width = ctx->fs_ptr ? ctx->fs_w : 0;
  *height = ctx->fs_ptr ? ctx->fs_h : 0;
  const int64_t m = ctx->fs_ptr ? std::min<int64_t>(capacity, (int64_t)ctx->fs_w * ctx->fs_h) : 0;
  if (m > 0) {
    BS_HIP(ctx, hipSetDevice(ctx->device));
    BS_HIP(ctx, hipMemcpyAsync(keep, ctx->fs_ptr, (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
    BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return BS_OK;
}

int bs_set_audit(bs_ctx* ctx, int on)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->audit = on ? 1 : 0;
  return BS_OK;
}

int bs_selftest_grow_limits(bs_ctx* ctx, const bs_grow_limits* lim)
{
  if (!ctx)
    return BS_ERR_INVALID;
  const bs_grow_limits none = {0, 0, 0, 0, -1, -1, 0, 0};
  if (lim && (lim->max_waves < 0 || lim->pool_cap < 0 || lim->max_pending < 0 || lim->pstore_cap < 0))
    return fail(ctx, BS_ERR_INVALID, "bs_selftest_grow_limits: a capacity is negative (0 = default)");
  ctx->lim = lim ? *lim : none;
  return BS_OK;
}

int bs_get_grow_counters(const bs_ctx* ctx, bs_grow_counters* out)
{
  if (!ctx || !out)
    return BS_ERR_INVALID;
  *out = ctx->gc;
  return BS_OK;
}

// ---- scratch guard (test hook) ----------------------------------------------
namespace {

struct ScratchMember {
  const char* name;
  int index;  // -1: a single buffer
  DevBuf* dev;
  HostBuf* host;
};

// EVERY DevBuf / HostBuf member of bs_ctx, in its order.  scratch_members_complete() counts the buffers a bs_ctx
// constructs against this table: a member added to bs_ctx and not listed here fails bs_create.
void scratch_members(bs_ctx* c, std::vector<ScratchMember>& out)
{
#define BS_ONE(m) out.push_back(ScratchMember{#m, -1, &c->m, nullptr})
#define BS_ARR(m)                                                  \
  for (int i = 0; i < (int)(sizeof(c->m) / sizeof(c->m[0])); i++) \
  out.push_back(ScratchMember{#m, i, &c->m[i], nullptr})
  BS_ONE(keys_in); BS_ONE(keys_out); BS_ONE(vals_in); BS_ONE(vals_out); BS_ONE(cub_tmp); BS_ONE(uniq_keys);
  BS_ONE(uniq_cnt); BS_ONE(misc); BS_ONE(table); BS_ONE(spts);
  BS_ONE(fb_list); BS_ONE(d_xyz_h); BS_ONE(d_neigh_h); BS_ONE(d_normals_h); BS_ONE(d_plane_h);
  BS_ONE(seg_neigh); BS_ONE(seg_normals);
  BS_ONE(rg_list); BS_ONE(rg_stack); BS_ONE(rg_planes); BS_ONE(rg_stats); BS_ONE(rg_aux); BS_ONE(rg_pstore);
  BS_ONE(rg_rec); BS_ONE(rg_radj); BS_ONE(rg_roff); BS_ONE(rg_geo); BS_ONE(rg_gs); BS_ONE(rg_disp);
  out.push_back(ScratchMember{"rg_hout", -1, nullptr, &c->rg_hout});
  BS_ONE(rs_keys_in); BS_ONE(rs_keys_out); BS_ONE(rs_vals_in); BS_ONE(rs_vals_out); BS_ONE(rs_cnt); BS_ONE(rs_img);
  BS_ONE(rs_tmp);
  BS_ONE(seg_npos);
  BS_ARR(fp); BS_ARR(bd); BS_ARR(rf); BS_ARR(ft); BS_ARR(sd); BS_ARR(fc); BS_ARR(ol); BS_ARR(sp); BS_ARR(uc); BS_ARR(sw);
  BS_ARR(tr); BS_ARR(ps); BS_ARR(mr); BS_ARR(pr); BS_ARR(gn);
  BS_ONE(bases_dev);
  BS_ARR(tn); BS_ARR(gd);
  BS_ONE(gm_dev);
  BS_ARR(evd); BS_ARR(hl);
  BS_ONE(fs_dev);
  BS_ARR(sh); BS_ARR(bt);
  BS_ONE(tile_desc);
#undef BS_ONE
#undef BS_ARR
}

// bs_ctx constructs exactly the buffers the table lists (no device needed: a context's constructor calls no HIP)
bool scratch_members_complete(bs_ctx* c, long long born, int64_t* n_members)
{
  std::vector<ScratchMember> m;
  scratch_members(c, m);
  if (n_members)
    *n_members = (int64_t)m.size();
  return born == (long long)m.size();
}

void scratch_slot(const ScratchMember& m, bs_scratch_slot* s)
{
  memset(s, 0, sizeof *s);
  if (m.index < 0)
    snprintf(s->name, sizeof s->name, "%s", m.name);
  else
    snprintf(s->name, sizeof s->name, "%s[%d]", m.name, m.index);
  s->address = (uint64_t)(uintptr_t)(m.dev ? m.dev->p : m.host->p);
  s->requested = (int64_t)(m.dev ? m.dev->cap : m.host->cap);
  s->guard = (int64_t)(m.dev ? m.dev->guard : m.host->guard);
  s->first_bad = s->last_bad = -1;
  s->host = m.host ? 1 : 0;
}

}  // namespace

int bs_selftest_scratch_guard(bs_ctx* ctx, int flags, int poison_byte)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if ((flags & ~(BS_SCRATCH_CANARY | BS_SCRATCH_POISON)) || poison_byte < 0 || poison_byte > 255)
    return fail(ctx, BS_ERR_INVALID, "bs_selftest_scratch_guard: flags are BS_SCRATCH_CANARY | BS_SCRATCH_POISON, the poison a byte");
  std::vector<ScratchMember> m;
  scratch_members(ctx, m);
  for (const auto& b : m)
    if (b.dev ? b.dev->p != nullptr : b.host->p != nullptr)
      return fail(ctx, BS_ERR_INVALID, "bs_selftest_scratch_guard: the context has already allocated (set the guard right after bs_create)");
  ctx->sg.flags = flags;
  ctx->sg.poison = (unsigned char)poison_byte;
  for (const auto& b : m) {
    if (b.dev)
      b.dev->sg = &ctx->sg;
    else
      b.host->sg = &ctx->sg;
  }
  return BS_OK;
}

int bs_selftest_scratch_list(bs_ctx* ctx, bs_scratch_slot* slots, int64_t capacity, int64_t* n_slots)
{
  if (!n_slots || capacity < 0 || (capacity > 0 && !slots))
    return BS_ERR_INVALID;
  *n_slots = 0;
  if (!ctx) {  // the member table against what a context constructs
    const long long before = scratch_bufs_born;
    bs_ctx* c = new (std::nothrow) bs_ctx();
    if (!c)
      return BS_ERR_NOMEM;
    const bool ok = scratch_members_complete(c, scratch_bufs_born - before, n_slots);
    delete c;
    return ok ? BS_OK : BS_ERR_INTERNAL;
  }
  std::vector<ScratchMember> m;
  scratch_members(ctx, m);
  for (const auto& b : m) {
    if ((b.dev ? b.dev->guard : b.host->guard) == 0)
      continue;
    if (*n_slots < capacity)
      scratch_slot(b, &slots[*n_slots]);
    ++*n_slots;
  }
  return BS_OK;
}

int bs_selftest_scratch_check(bs_ctx* ctx, bs_scratch_report* rep)
{
  if (!ctx || !rep)
    return BS_ERR_INVALID;
  memset(rep, 0, sizeof *rep);
  BS_HIP(ctx, hipSetDevice(ctx->device));
  BS_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->side)
    BS_HIP(ctx, hipStreamSynchronize(ctx->side));
  std::vector<ScratchMember> m;
  scratch_members(ctx, m);
  std::vector<unsigned char> h;
  for (const auto& b : m) {
    const size_t g = b.dev ? b.dev->guard : b.host->guard;
    if (g == 0)
      continue;
    const size_t req = b.dev ? b.dev->cap : b.host->cap;
    rep->n_guarded++;
    rep->bytes_requested += (int64_t)req;
    if (!(ctx->sg.flags & BS_SCRATCH_CANARY))  // (poison alone: the guards hold nothing to compare)
      continue;
    const unsigned char* v;
    if (b.dev) {
      h.resize(g);
      BS_HIP(ctx, hipMemcpy(h.data(), (const char*)b.dev->p + req, g, hipMemcpyDeviceToHost));
      v = h.data();
    } else {
      v = (const unsigned char*)b.host->p + req;
    }
    int64_t first = -1, last = -1;
    for (size_t i = 0; i < g; i++)
      if (v[i] != SCRATCH_CANARY) {
        if (first < 0)
          first = (int64_t)i;
        last = (int64_t)i;
      }
    if (first < 0)
      continue;
    if (rep->n_damaged < BS_SCRATCH_REPORT_MAX) {
      bs_scratch_slot* s = &rep->damaged[rep->n_damaged];
      scratch_slot(b, s);
      s->first_bad = first;
      s->last_bad = last;
      rep->n_listed++;
    }
    rep->n_damaged++;
  }
  return BS_OK;
}

int bs_planes_fetch(bs_ctx* ctx, bs_planes* out)
{
  if (!ctx || !out)
    return BS_ERR_INVALID;
  memset(out, 0, sizeof *out);
  if (!ctx->rg_valid)
    return fail(ctx, BS_ERR_INVALID, "no region-grow result on this context");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  GrowStats hs;
  BS_HIP(ctx, hipMemcpy(&hs, ctx->rg_stats.p, sizeof hs, hipMemcpyDeviceToHost));
  return planes_to_host(ctx, ctx->rg_planes.as<PlaneRec>(), ctx->rg_list.as<int32_t>(), hs.n_planes, hs.list_used, out);
}

void bs_planes_free(bs_planes* p)
{
  if (!p)
    return;
  free(p->id);
  free(p->normal);
  free(p->center);
  free(p->offset);
  free(p->point_idx);
  memset(p, 0, sizeof *p);
}

int bs_plane_colors(const bs_planes* planes, const int32_t* plane_rgb, int64_t n, uint16_t* colors)
{
  if (!planes || !colors || n < 0 || (planes->n_planes > 0 && !plane_rgb))
    return BS_ERR_INVALID;
  memset(colors, 0, sizeof(uint16_t) * 3 * (size_t)n);  // my_function.cpp:262-264
  for (int p = 0; p < planes->n_planes; p++) {          // :268-274
    for (int64_t t = planes->offset[p]; t < planes->offset[p + 1]; t++) {
      const int32_t id = planes->point_idx[t];
      if (id < 0 || id >= n)
        return BS_ERR_INVALID;
      for (int a = 0; a < 3; a++)
        colors[3 * (int64_t)id + a] = (uint16_t)plane_rgb[3 * p + a];
    }
  }
  return BS_OK;
}

// ---------------------------------------------------------------------------
// host-buffer entry points (stage through context-owned device buffers)
// ---------------------------------------------------------------------------

int bs_knn_normals(bs_ctx* ctx, const int32_t* xyz, int64_t n, const bs_params* p, int32_t* neigh,
                   double* normals)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!xyz || !neigh || !normals)
    return fail(ctx, BS_ERR_INVALID, "null host pointer");
  int rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(ctx->d_xyz_h, xyz, 3 * n);
  int32_t* d_neigh = S.room<int32_t>(ctx->d_neigh_h, n * p->k);
  double* d_normals = S.room<double>(ctx->d_normals_h, 3 * n);
  if (!S.ok())
    return S.status();
  rc = bs_knn_normals_dev(ctx, d_xyz, nullptr, n, 0, n, p, d_neigh, d_normals, 0.0, nullptr);
  if (rc != BS_OK)
    return rc;
  S.download(neigh, d_neigh, n * p->k);
  S.download(normals, d_normals, 3 * n);
  return S.finish();
}

int bs_knn_normals_halo(bs_ctx* ctx, const int32_t* xyz, const int32_t* gidx, int64_t n, int64_t n_query,
                        const bs_params* p, int32_t* neigh, double* normals, double cert_radius,
                        int64_t* n_uncertified)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!xyz || !gidx || !neigh || !normals)
    return fail(ctx, BS_ERR_INVALID, "null host pointer");
  int rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  if (n_query < 0 || n_query > n)
    return fail(ctx, BS_ERR_INVALID, "bad n_query");
  for (int64_t i = 0; i < n; i++)
    if (gidx[i] < 0)
      return fail(ctx, BS_ERR_INVALID, "negative global index");
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(ctx->d_xyz_h, xyz, 3 * n);
  const int32_t* d_gidx = S.upload(ctx->d_plane_h, gidx, n);  // (the labels' slot: this call has none)
  int32_t* d_neigh = S.room<int32_t>(ctx->d_neigh_h, std::max<int64_t>(n_query, 1) * p->k);
  double* d_normals = S.room<double>(ctx->d_normals_h, 3 * std::max<int64_t>(n_query, 1));
  if (!S.ok())
    return S.status();
  rc = bs_knn_normals_dev(ctx, d_xyz, d_gidx, n, 0, n_query, p, d_neigh, d_normals, cert_radius, n_uncertified);
  if (rc != BS_OK)
    return rc;
  S.download(neigh, d_neigh, n_query * p->k);
  S.download(normals, d_normals, 3 * n_query);
  return S.finish();
}

int bs_region_grow(bs_ctx* ctx, const int32_t* xyz, const double* normals, const int32_t* neigh, int64_t n,
                   const bs_params* p, int32_t* plane_idx, bs_planes* planes)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (planes)
    memset(planes, 0, sizeof *planes);
  if (!xyz || !normals || !neigh || !plane_idx)
    return fail(ctx, BS_ERR_INVALID, "null host pointer");
  int rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  // neighbour indices are dereferenced on the device: validate them here
  for (int64_t i = 0; i < n * (int64_t)p->k; i++)
    if (neigh[i] < 0 || neigh[i] >= n)
      return fail(ctx, BS_ERR_INVALID, "neighbour index out of range");
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(ctx->d_xyz_h, xyz, 3 * n);
  const int32_t* d_neigh = S.upload(ctx->d_neigh_h, neigh, n * p->k);
  const double* d_normals = S.upload(ctx->d_normals_h, normals, 3 * n);
  int32_t* d_plane = S.room<int32_t>(ctx->d_plane_h, n);
  if (!S.ok())
    return S.status();
  ctx->npos_neigh = nullptr;  // the staging buffers now hold the caller's data, not what a previous bs_segment searched
  ctx->npos_normals = nullptr;
  rc = region_grow_dev_impl(ctx, d_xyz, d_normals, d_neigh, n, p, d_plane, true);
  if (rc != BS_OK)
    return rc;
  S.download(plane_idx, d_plane, n);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  if (planes)
    return bs_planes_fetch(ctx, planes);
  return BS_OK;
}

int bs_segment(bs_ctx* ctx, const int32_t* xyz, int64_t n, const bs_params* p, int32_t* neigh, double* normals,
               int32_t* plane_idx, bs_planes* planes)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (planes)
    memset(planes, 0, sizeof *planes);
  if (!xyz || !plane_idx)
    return fail(ctx, BS_ERR_INVALID, "null host pointer");
  int rc = check_params(ctx, p, n);
  if (rc != BS_OK)
    return rc;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(ctx->d_xyz_h, xyz, 3 * n);
  int32_t* d_neigh = S.room<int32_t>(ctx->d_neigh_h, n * p->k);
  double* d_normals = S.room<double>(ctx->d_normals_h, 3 * n);
  int32_t* d_plane = S.room<int32_t>(ctx->d_plane_h, n);
  if (!S.ok())
    return S.status();
  rc = bs_segment_dev(ctx, d_xyz, n, p, d_neigh, d_normals, d_plane);
  if (rc != BS_OK)
    return rc;
  S.download(neigh, d_neigh, n * p->k);
  S.download(normals, d_normals, 3 * n);
  S.download(plane_idx, d_plane, n);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  if (planes)
    return bs_planes_fetch(ctx, planes);
  return BS_OK;
}

}  // extern "C"
