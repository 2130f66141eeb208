// bs_facet.hip -- the roof facets of every building and the edges between them (DESIGN.md "Roof facets"; the definition
// is written down in include/bs_api.h under "roof facets").
//   label    union-find in two levels over the image, 4-connected, for an arbitrary 64-bit class (building << 32 | plane):
//            one workgroup per TW x TH tile, a row of a tile is one wave.  The start of a lane's run comes from ONE ballot
//            of "differs from the lane to my left"; only the vertical links go through LDS atomics.  Every pixel gets the
//            GLOBAL index of its tile-component's first pixel; a seam kernel unites across tile edges with bs_uf.h; one
//            flatten pass.  parent <= self throughout, so a root is its facet's first raster pixel.  The range checks
//            ride on the tile kernel: nothing of the caller's is written before they have passed.
//   number   roots flagged and scanned (hipcub): facet = rank of the root = ascending start pixel; the facet image
//   figures  one pixel pass: the inner and outer sides of every pixel, its border flags (direction 0 and 1) as one byte,
//            and the per-facet figures reduced over runs of equal facet inside a wave (a segmented scan over the ballot
//            of run heads) before ONE set of global atomics per run -- facet ids are unbounded, no LDS table holds them
//   edges    border flags scanned; one 64-bit key (facet_lo << 32 | facet_hi) and the pixel-edge number 2 * pixel +
//            direction per border edge; radix sort of the pairs; run heads scanned = the edge of every sorted item; the
//            figures of a border edge recomputed from top by its number and reduced over runs inside a wave as above
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <vector>

#include "bs_common.h"
#include "bs_facet_dev.h"
#include "bs_segscan.h"
#include "bs_uf.h"

namespace bs {
namespace {

constexpr int TW = 64, TH = 16;  // labelling tile (the kernels are in bs_facet_dev.h)
static_assert(TW == LABEL_TW && TH == LABEL_TH, "the labelling tile of bs_facet_dev.h");
// scratch of bs_ctx::fc
enum { FC_PARENT, FC_SCAN, FC_FLAGS, FC_TMP, FC_MISC, FC_FFIG, FC_KEYS, FC_KEYS2, FC_VALS, FC_VALS2, FC_EID, FC_EFIG, FC_IN_MAP,
       FC_IN_ROOF, FC_IN_TOP, FC_FACET };

// (every array is allocated even after a failure: bs_roof_facets_free takes them all)
bool alloc_facets(struct bs_roof_facets* s, size_t nf)
{
  const bool ok[] = {alloc(&s->facet_building, nf),    alloc(&s->facet_plane, nf),       alloc(&s->facet_start_xy, 2 * nf),
                     alloc(&s->facet_pixels, nf),      alloc(&s->facet_bbox, 4 * nf),    alloc(&s->facet_inner_edges, nf),
                     alloc(&s->facet_outer_edges, nf), alloc(&s->facet_top_min, nf),     alloc(&s->facet_top_max, nf),
                     alloc(&s->facet_top_sum, nf)};
  return std::all_of(std::begin(ok), std::end(ok), [](bool b) { return b; });
}

bool alloc_edges(struct bs_roof_facets* s, size_t ne)
{
  const bool ok[] = {alloc(&s->edge_facet, 2 * ne),     alloc(&s->edge_building, ne),     alloc(&s->edge_length, ne),
                     alloc(&s->edge_n_dir0, ne),        alloc(&s->edge_n_step, ne),       alloc(&s->edge_step_abs_sum, ne),
                     alloc(&s->edge_step_abs_max, ne),  alloc(&s->edge_rise_sum, ne),     alloc(&s->edge_bend_sum, ne),
                     alloc(&s->edge_z_min, ne),         alloc(&s->edge_z_max, ne),        alloc(&s->edge_bbox, 4 * ne)};
  return std::all_of(std::begin(ok), std::end(ok), [](bool b) { return b; });
}

using Guard = FreeUnlessKept<struct bs_roof_facets, bs_roof_facets_free>;

// (a pixel edge is numbered 2 * pixel + direction in 32 bits)
bool bad_image(int32_t w, int32_t h) { return w < 1 || h < 1 || (int64_t)w * h >= (1ll << 30); }

const char* const FACETS_INVALID = "roof facets: null pointer, width or height < 1, width * height >= 2^30, n_buildings or "
                                   "n_planes < 0, or d_top not 16-byte aligned";

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_roof_facets_free(struct bs_roof_facets* s)
{
  if (!s)
    return;
  free(s->facet_building);
  free(s->facet_plane);
  free(s->facet_start_xy);
  free(s->facet_pixels);
  free(s->facet_bbox);
  free(s->facet_inner_edges);
  free(s->facet_outer_edges);
  free(s->facet_top_min);
  free(s->facet_top_max);
  free(s->facet_top_sum);
  free(s->edge_facet);
  free(s->edge_building);
  free(s->edge_length);
  free(s->edge_n_dir0);
  free(s->edge_n_step);
  free(s->edge_step_abs_sum);
  free(s->edge_step_abs_max);
  free(s->edge_rise_sum);
  free(s->edge_bend_sum);
  free(s->edge_z_min);
  free(s->edge_z_max);
  free(s->edge_bbox);
  memset(s, 0, sizeof *s);
}

extern "C" int bs_roof_facets_dev(bs_ctx* ctx, const int32_t* d_map, const int32_t* d_roof, const int32_t* d_top,
                                  int32_t width, int32_t height, int32_t n_buildings, int32_t n_planes, int32_t* d_facet,
                                  struct bs_roof_facets* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_map || !d_roof || !d_top || !d_facet || !out || bad_image(width, height) || n_buildings < 0 || n_planes < 0 ||
      (reinterpret_cast<uintptr_t>(d_top) & 15u))  // (the four tops of a pixel are one 16-byte load)
    return fail(ctx, BS_ERR_INVALID, FACETS_INVALID);
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int w = width, h = height;
  const int64_t npix = (int64_t)w * h;
  const int ntx = nblk(w, TW), nty = nblk(h, TH);
  DevBuf* B = ctx->fc;
  const int4* top = reinterpret_cast<const int4*>(d_top);
  const Cls cls{d_map, d_roof};
  Events<11> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));

  hipcub::CountingInputIterator<int32_t> idx(0);
  BS_HIP(ctx, B[FC_PARENT].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[FC_SCAN].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[FC_FLAGS].reserve((size_t)npix));
  BS_HIP(ctx, B[FC_MISC].reserve(256));
  int32_t* parent = B[FC_PARENT].as<int32_t>();
  int32_t* scan = B[FC_SCAN].as<int32_t>();  // ranks of the roots, then the offsets of the border edges
  uint8_t* flags = B[FC_FLAGS].as<uint8_t>();
  int* d_bad = B[FC_MISC].as<int>();
  hipcub::TransformInputIterator<int32_t, RootFlag, hipcub::CountingInputIterator<int32_t>> roots(idx, RootFlag{parent});
  auto number = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, roots, scan, (int)npix, st); };
  auto offsets = [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, FlagIt(flags, FlagCount()), scan, (int)npix, st);
  };
  BS_HIP(ctx, cub_room(B[FC_TMP], number, offsets));

  // ---- label (into the context: nothing of the caller's is written before the checks have passed) ----
  BS_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, st));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  facet_tile_kernel<<<ntx * nty, 256, 0, st>>>(cls, w, h, ntx, n_buildings, n_planes, parent, d_bad);
  {
    const int64_t n_h = (int64_t)(nty - 1) * w, total = n_h + (int64_t)(ntx - 1) * h;
    if (total > 0)
      facet_seam_kernel<<<nblk(total, 256), 256, 0, st>>>(cls, w, h, n_h, total, parent);
  }
  facet_flatten_kernel<<<nblk(npix, 256), 256, 0, st>>>(parent, npix);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  // ---- number ----
  BS_HIP(ctx, cub_run(B[FC_TMP], number));
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  int h_bad = 0;
  int32_t last_rank = 0, last_parent = -1;
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_rank, scan + npix - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_parent, parent + npix - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_bad)
    return fail(ctx, BS_ERR_RANGE,
                "roof facets: a map value >= n_buildings, a roof value > n_planes, or a roof > 0 outside every building");
  const int64_t nf = (int64_t)last_rank + (last_parent == (int32_t)(npix - 1));

  struct bs_roof_facets res;
  memset(&res, 0, sizeof res);
  Guard guard{&res};
  if (!alloc_facets(&res, (size_t)nf))
    return fail(ctx, BS_ERR_NOMEM, "roof facets: host allocation");
  BS_HIP(ctx, B[FC_FFIG].reserve(FACET_FIG_BYTES * (size_t)std::max<int64_t>(nf, 1)));
  const FacetFig F = facet_fig_at(B[FC_FFIG].p, (size_t)std::max<int64_t>(nf, 1));
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  if (nf > 0)
    facet_fig_init_kernel<<<nblk(nf, 256), 256, 0, st>>>(F, nf);
  facet_write_kernel<<<nblk(npix, 256), 256, 0, st>>>(parent, scan, npix, d_facet);
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  // ---- figures ----
  facet_figures_kernel<<<grid_of(npix), 256, 0, st>>>(d_map, d_roof, top, parent, d_facet, w, h, flags, F);
  BS_HIP(ctx, hipEventRecord(ev.e[5], st));
  // ---- edges: at most 2 * width * height < 2^31 border edges (the check on the image), so every sum below fits 32 bits ----
  BS_HIP(ctx, cub_run(B[FC_TMP], offsets));
  BS_HIP(ctx, hipEventRecord(ev.e[6], st));
  int32_t last_off = 0;
  uint8_t last_flag = 0;
  BS_HIP(ctx, hipMemcpyAsync(&last_off, scan + npix - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_flag, flags + npix - 1, 1, hipMemcpyDeviceToHost, st));
  if (nf > 0) {
    const size_t n = (size_t)nf;
    BS_HIP(ctx, hipMemcpyAsync(res.facet_pixels, F.pixels, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_inner_edges, F.inner, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_outer_edges, F.outer, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_top_sum, F.top_sum, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_bbox, F.bbox, 16 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_top_min, F.top_min, 4 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_top_max, F.top_max, 4 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_building, F.building, 4 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_plane, F.plane, 4 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.facet_start_xy, F.start_xy, 8 * n, hipMemcpyDeviceToHost, st));
  }
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  const int64_t nbord = (int64_t)last_off + (last_flag & 1) + (last_flag >> 1);
  int64_t ne = 0;
  double ms_sort = 0, ms_reduce = 0;
  if (nbord > 0) {
    const int nbi = (int)nbord;
    const int end_bit = 32 + bits_of(nf);
    BS_HIP(ctx, B[FC_KEYS].reserve(8 * (size_t)nbord));
    BS_HIP(ctx, B[FC_KEYS2].reserve(8 * (size_t)nbord));
    BS_HIP(ctx, B[FC_VALS].reserve(4 * (size_t)nbord));
    BS_HIP(ctx, B[FC_VALS2].reserve(4 * (size_t)nbord));
    BS_HIP(ctx, B[FC_EID].reserve(4 * (size_t)nbord));
    unsigned long long* keys = B[FC_KEYS].as<unsigned long long>();
    unsigned long long* sorted = B[FC_KEYS2].as<unsigned long long>();
    int32_t* vals = B[FC_VALS].as<int32_t>();
    int32_t* svals = B[FC_VALS2].as<int32_t>();
    int32_t* eid = B[FC_EID].as<int32_t>();
    hipcub::TransformInputIterator<int32_t, HeadFlag, hipcub::CountingInputIterator<int32_t>> heads(idx, HeadFlag{sorted});
    auto sort = [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, sorted, vals, svals, nbi, 0, end_bit, st);
    };
    auto ids = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::InclusiveSum(tmp, bytes, heads, eid, nbi, st); };
    BS_HIP(ctx, cub_room(B[FC_TMP], sort, ids));
    BS_HIP(ctx, hipEventRecord(ev.e[7], st));
    edge_emit_kernel<<<grid_of(npix), 256, 0, st>>>(flags, scan, d_facet, w, npix, keys, vals);
    BS_HIP(ctx, cub_run(B[FC_TMP], sort));
    BS_HIP(ctx, cub_run(B[FC_TMP], ids));
    BS_HIP(ctx, hipEventRecord(ev.e[8], st));
    int32_t h_ne = 0;
    BS_HIP(ctx, hipMemcpyAsync(&h_ne, eid + nbord - 1, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    BS_HIP(ctx, hipGetLastError());
    ne = h_ne;
    if (!alloc_edges(&res, (size_t)ne))
      return fail(ctx, BS_ERR_NOMEM, "roof facets: host allocation");
    BS_HIP(ctx, B[FC_EFIG].reserve(EDGE_FIG_BYTES * (size_t)ne));
    const EdgeFig E = edge_fig_at(B[FC_EFIG].p, (size_t)ne);
    BS_HIP(ctx, hipEventRecord(ev.e[9], st));
    edge_fig_init_kernel<<<nblk(ne, 256), 256, 0, st>>>(E, ne);
    edge_reduce_kernel<<<grid_of(nbord), 256, 0, st>>>(sorted, svals, eid, nbord, d_map, top, d_facet, w, E);
    BS_HIP(ctx, hipEventRecord(ev.e[10], st));
    const size_t n = (size_t)ne;
    BS_HIP(ctx, hipMemcpyAsync(res.edge_length, E.length, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_n_dir0, E.n_dir0, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_n_step, E.n_step, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_step_abs_sum, E.step_abs_sum, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_step_abs_max, E.step_abs_max, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_rise_sum, E.rise_sum, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_bend_sum, E.bend_sum, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_facet, E.facet, 8 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_building, E.building, 4 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_z_min, E.z_min, 4 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_z_max, E.z_max, 4 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(res.edge_bbox, E.bbox, 16 * n, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    BS_HIP(ctx, hipGetLastError());
    ms_sort = ev.ms(7, 8);
    ms_reduce = ev.ms(9, 10);
  } else if (!alloc_edges(&res, 0)) {
    return fail(ctx, BS_ERR_NOMEM, "roof facets: host allocation");
  }
  int64_t npx = 0;
  for (int64_t k = 0; k < nf; k++)
    npx += res.facet_pixels[k];
  res.width = w;
  res.height = h;
  res.n_facets = nf;
  res.n_edges = ne;
  res.n_pixels = npx;
  res.n_border = nbord;
  res.ms_label = ev.ms(0, 1);
  res.ms_number = ev.ms(1, 2) + ev.ms(3, 4);
  res.ms_figures = ev.ms(4, 5);
  res.ms_edges = ev.ms(5, 6) + ms_sort + ms_reduce;
  *out = res;
  guard.keep = true;
  return BS_OK;
}

extern "C" int bs_roof_facets(bs_ctx* ctx, const int32_t* map, const int32_t* roof, const int32_t* top, int32_t width,
                              int32_t height, int32_t n_buildings, int32_t n_planes, int32_t* facet,
                              struct bs_roof_facets* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!map || !roof || !top || !facet || !out || bad_image(width, height) || n_buildings < 0 || n_planes < 0)
    return fail(ctx, BS_ERR_INVALID, FACETS_INVALID);
  const size_t npix = (size_t)width * height;
  DevBuf* B = ctx->fc;
  Staging S(ctx);
  const int32_t* d_map = S.upload(B[FC_IN_MAP], map, npix);
  const int32_t* d_roof = S.upload(B[FC_IN_ROOF], roof, npix);
  const int32_t* d_top = S.upload(B[FC_IN_TOP], top, 4 * npix);
  int32_t* d_facet = S.room<int32_t>(B[FC_FACET], npix);
  if (!S.ok())
    return S.status();
  struct bs_roof_facets res;
  int rc = bs_roof_facets_dev(ctx, d_map, d_roof, d_top, width, height, n_buildings, n_planes, d_facet, &res);
  if (rc != BS_OK)
    return rc;
  Guard guard{&res};
  S.download(facet, d_facet, npix);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  *out = res;
  return BS_OK;
}

// The rules are written down in include/bs_api.h.
extern "C" int bs_roof_edge_kinds(const struct bs_roof_facets* f, int32_t step_tol, int32_t bend_tol, uint8_t* kind_out)
{
  if (!f || !kind_out || step_tol < 0 || bend_tol < 0 || f->n_edges < 0)
    return BS_ERR_INVALID;
  if (f->n_edges > 0 && (!f->edge_length || !f->edge_step_abs_sum || !f->edge_bend_sum))
    return BS_ERR_INVALID;
  for (int64_t e = 0; e < f->n_edges; e++) {
    const int64_t len = f->edge_length[e];
    uint8_t k = 0;
    if (f->edge_step_abs_sum[e] > 2 * (int64_t)step_tol * len)
      k = 3;
    else if (f->edge_bend_sum[e] > (int64_t)bend_tol * len)
      k = 1;
    else if (f->edge_bend_sum[e] < -(int64_t)bend_tol * len)
      k = 2;
    kind_out[e] = k;
  }
  return BS_OK;
}

// The format is written down in include/bs_api.h.
extern "C" int bs_roof_edges_write_obj(const int32_t* facet, const int32_t* map, const int32_t* top, int32_t width,
                                       int32_t height, int32_t bin, const struct bs_roof_facets* f, const uint8_t* kind,
                                       const int32_t* origin, const char* path)
{
  if (!facet || !map || !top || !f || !kind || !path || bin < 1 || bad_image(width, height) || f->n_edges < 0 ||
      (f->n_edges > 0 && !f->edge_facet))
    return BS_ERR_INVALID;
  const int w = width, h = height;
  const int64_t ne = f->n_edges;
  for (int64_t e = 0; e < ne; e++)
    if (kind[e] > 3)
      return BS_ERR_INVALID;
  // the edge of a facet pair: binary search in the ascending (lo, hi) list
  auto edge_of = [&](int32_t fa, int32_t fb) -> int64_t {
    const int32_t lo = std::min(fa, fb), hi = std::max(fa, fb);
    int64_t a = 0, b = ne;
    while (a < b) {
      const int64_t m = (a + b) / 2;
      const int32_t mlo = f->edge_facet[2 * m], mhi = f->edge_facet[2 * m + 1];
      if (mlo < lo || (mlo == lo && mhi < hi))
        a = m + 1;
      else
        b = m;
    }
    return (a < ne && f->edge_facet[2 * a] == lo && f->edge_facet[2 * a + 1] == hi) ? a : -1;
  };
  // the border edges in ascending (y, x, direction), then a stable counting sort by edge
  std::vector<int32_t> seg, seg_edge;
  std::vector<int64_t> first((size_t)ne + 1, 0);
  for (int64_t i = 0; i < (int64_t)w * h; i++) {
    const int32_t c = map[i];
    if (c < 0)
      continue;
    const int x = (int)(i % w), y = (int)(i / w);
    for (int d = 0; d < 2; d++) {
      if (d == 0 ? x + 1 >= w : y + 1 >= h)
        continue;
      const int64_t q = i + (d ? w : 1);
      if (map[q] != c || facet[q] == facet[i])
        continue;
      const int64_t e = edge_of(facet[i], facet[q]);
      if (e < 0)
        return BS_ERR_INVALID;
      seg.push_back((int32_t)(2 * i + d));
      seg_edge.push_back((int32_t)e);
      first[(size_t)e + 1]++;
    }
  }
  for (int64_t e = 0; e < ne; e++)
    first[(size_t)e + 1] += first[(size_t)e];
  std::vector<int32_t> order(seg.size());
  {
    std::vector<int64_t> at(first.begin(), first.end() - 1);
    for (size_t k = 0; k < seg.size(); k++)
      order[(size_t)at[seg_edge[k]]++] = seg[k];
  }
  FILE* fo = fopen(path, "w");
  if (!fo)
    return BS_ERR_INVALID;
  static const char* const NAMES[4] = {"flat", "ridge", "valley", "step"};
  const int64_t o[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  fprintf(fo, "# roof edges: %lld edges, %lld segments\n", (long long)ne, (long long)seg.size());
  long long nv = 0;
  for (int64_t e = 0; e < ne; e++) {
    fprintf(fo, "g edge_%lld_%s\n", (long long)e, NAMES[kind[e]]);
    for (int64_t k = first[(size_t)e]; k < first[(size_t)e + 1]; k++) {
      const int32_t v = order[(size_t)k];
      const int64_t a = v >> 1, b = a + ((v & 1) ? w : 1);
      const int d = v & 1, x = (int)(a % w), y = (int)(a / w);
      const int32_t* A = top + 4 * a;
      const int32_t* Bt = top + 4 * b;
      const int64_t zs = std::max(d ? A[2] : A[1], Bt[0]), ze = std::max(A[3], d ? Bt[1] : Bt[2]);
      const int64_t xs = d ? x : x + 1, ys = d ? y + 1 : y;
      fprintf(fo, "v %lld %lld %lld\n", (long long)(xs * bin + o[0]), (long long)(ys * bin + o[1]), (long long)(zs + o[2]));
      fprintf(fo, "v %lld %lld %lld\n", (long long)((int64_t)(x + 1) * bin + o[0]), (long long)((int64_t)(y + 1) * bin + o[1]),
              (long long)(ze + o[2]));
      fprintf(fo, "l %lld %lld\n", nv + 1, nv + 2);
      nv += 2;
    }
  }
  const bool ok = !ferror(fo);
  return (fclose(fo) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}
