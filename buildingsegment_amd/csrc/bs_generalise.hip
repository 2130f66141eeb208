// bs_generalise.hip -- roof generalisation: small facets and facets across a FLAT edge merged into their neighbours
// (DESIGN.md "Roof generalisation"; the definition is written down in include/bs_api.h under "roof generalisation").
//   evaluate  tops (bs_tops.h) and the facet passes (bs_facet_dev.h) of the current image on this stage's own scratch, then
//     rank        one radix sort of ((2^30 - pixels) << 32 | id): order[f] = the place of f, 0 = the highest rank
//     candidates  one thread per edge: its kind from length / step_abs_sum / bend_sum, the direction lower rank -> higher
//                 rank, at most ONE no-return 64-bit atomicMax of (length << 32 | (2^30 - 1 - order[g]) << 1 | reason) on
//                 best[f]; the FLAT edges counted by wave
//     resolve     best -> target (through the sorted ids), one link of chain, the movers / reasons / small facets / facets
//                 per building counted by wave
//     chain ends  pointer doubling, ceil(log2 n_facets) rounds over (next, links): no thread walks a chain
//     new plane   plane[end[f]] of every mover (0: stays) and the longest chain
//   apply     one pixel pass: facet -> new plane
//   figures   once, after the last evaluation: input image against the result and first tops against last tops; runs of
//             equal building reduced inside the wave (bs_segscan.h), LDS tables below BS_GEN_FIG_CAP / BS_GEN_PLANE_CAP,
//             global atomics above
// The caller's images are read only until everything has succeeded; then the result is copied out.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_common.h"
#include "bs_facet_dev.h"
#include "bs_segscan.h"
#include "bs_tops.h"

namespace bs {
namespace {

// scratch of bs_ctx::gn
enum { GN_ROOF, GN_CMAP, GN_TOP0, GN_TOP1, GN_PARENT, GN_SCAN, GN_FLAGS, GN_FACET, GN_TMP, GN_MISC, GN_TAB, GN_FFIG, GN_KEYS,
       GN_KEYS2, GN_VALS, GN_VALS2, GN_EID, GN_EFIG, GN_RKEY, GN_RKEY2, GN_ORDER, GN_BEST, GN_NEXT, GN_NEXT2, GN_DIST, GN_DIST2,
       GN_NEWP, GN_BFAC, GN_FIG, GN_IN_MAP, GN_IN_ROOF, GN_OUT };
// counters of GN_MISC (unsigned long long each)
enum { CN_BAD, CN_FLAT, CN_SMALL, CN_MOVERS, CN_MOVERS_SMALL, CN_MOVERS_FLAT, CN_CHAIN, CN_ROOFED, CN_COUNT };

constexpr unsigned ORDER_TOP = (1u << 30) - 1u;  // order < 2^30: width * height < 2^30

using ull = unsigned long long;

struct Rule {
  long long min_pixels;
  int merge_flat;
  long long step_tol, bend_tol;
};

// ---- rank ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rank_key_kernel(const ull* __restrict__ pixels, int64_t nf, ull* __restrict__ keys)
{
  const int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (f < nf)
    keys[f] = (((1ull << 30) - pixels[f]) << 32) | (ull)f;
}

__global__ __launch_bounds__(256) void order_kernel(const ull* __restrict__ sorted, int64_t nf, int32_t* __restrict__ order,
                                                    ull* __restrict__ best)
{
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (k >= nf)
    return;
  order[(uint32_t)sorted[k]] = (int32_t)k;
  best[k] = 0;
}

// ---- candidates ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void candidates_kernel(EdgeFig E, int64_t ne, const ull* __restrict__ pixels,
                                                         const int32_t* __restrict__ plane, const int32_t* __restrict__ order,
                                                         Rule r, ull* __restrict__ best, ull* __restrict__ counters)
{
  const int64_t ne64 = (ne + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < ne64; e += (int64_t)gridDim.x * blockDim.x) {
    bool flat = false;
    if (e < ne) {
      const long long len = (long long)E.length[e], asum = (long long)E.step_abs_sum[e], bend = (long long)E.bend_sum[e];
      flat = !(asum > 2 * r.step_tol * len) && !(bend > r.bend_tol * len) && !(bend < -r.bend_tol * len);
      const int32_t lo = E.facet[2 * e], hi = E.facet[2 * e + 1];
      const bool up = order[hi] < order[lo];  // hi outranks lo
      const int32_t f = up ? lo : hi, g = up ? hi : lo;
      const bool by_flat = r.merge_flat && flat;
      if (plane[g] > 0 && ((long long)pixels[f] < r.min_pixels || by_flat))
        atomicMax(best + f, ((ull)len << 32) | ((ull)(ORDER_TOP - (unsigned)order[g]) << 1) | (ull)by_flat);
    }
    const ull m = __ballot(flat);
    if ((threadIdx.x & 63) == 0 && m)
      atomicAdd(counters + CN_FLAT, (ull)__popcll(m));
  }
}

// ---- resolve ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void resolve_kernel(int64_t nf, const ull* __restrict__ best, const ull* __restrict__ sorted,
                                                      const ull* __restrict__ pixels, const int32_t* __restrict__ building,
                                                      long long min_pixels, int32_t* __restrict__ next,
                                                      int32_t* __restrict__ dist, ull* __restrict__ counters,
                                                      ull* __restrict__ bfac)
{
  const int lane = threadIdx.x & 63;
  const int64_t nf64 = (nf + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf64; f += (int64_t)gridDim.x * blockDim.x) {
    bool mover = false, by_flat = false, small = false;
    int32_t c = -1;
    if (f < nf) {
      const ull b = best[f];
      mover = b != 0;
      by_flat = mover && (b & 1ull);
      small = (long long)pixels[f] < min_pixels;
      c = building[f];
      next[f] = mover ? (int32_t)(uint32_t)sorted[ORDER_TOP - (unsigned)((b & 0xFFFFFFFFull) >> 1)] : (int32_t)f;
      dist[f] = mover;
    }
    const ull m_valid = __ballot(f < nf), m_mover = __ballot(mover), m_flat = __ballot(by_flat), m_small = __ballot(small);
    // facets per building: ids ascend with the start pixel, so a wave mostly holds one building
    const int32_t c0 = __shfl(c, 0);
    const bool uniform = __all(f >= nf || c == c0);
    if (!uniform && f < nf)
      atomicAdd(bfac + c, 1ull);
    if (lane == 0) {
      if (uniform)
        atomicAdd(bfac + c0, (ull)__popcll(m_valid));
      if (m_mover) {
        atomicAdd(counters + CN_MOVERS, (ull)__popcll(m_mover));
        if (m_flat)
          atomicAdd(counters + CN_MOVERS_FLAT, (ull)__popcll(m_flat));
        if (m_mover & ~m_flat)
          atomicAdd(counters + CN_MOVERS_SMALL, (ull)__popcll(m_mover & ~m_flat));
      }
      if (m_small)
        atomicAdd(counters + CN_SMALL, (ull)__popcll(m_small));
    }
  }
}

// ---- chain ends ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void double_kernel(int64_t nf, const int32_t* __restrict__ next,
                                                     const int32_t* __restrict__ dist, int32_t* __restrict__ next2,
                                                     int32_t* __restrict__ dist2)
{
  const int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (f >= nf)
    return;
  const int32_t n = next[f];
  next2[f] = next[n];
  dist2[f] = dist[f] + dist[n];
}

__global__ __launch_bounds__(256) void new_plane_kernel(int64_t nf, const int32_t* __restrict__ end,
                                                        const int32_t* __restrict__ dist, const int32_t* __restrict__ plane,
                                                        int32_t* __restrict__ newp, ull* __restrict__ counters)
{
  const int64_t nf64 = (nf + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t f = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; f < nf64; f += (int64_t)gridDim.x * blockDim.x) {
    int32_t d = 0;
    if (f < nf) {
      const int32_t e = end[f];
      newp[f] = e != (int32_t)f ? plane[e] : 0;  // (a target has a plane > 0: 0 says "stays")
      d = dist[f];
    }
    for (int o = 32; o > 0; o >>= 1)
      d = max(d, __shfl_xor(d, o));
    if ((threadIdx.x & 63) == 0 && d)
      atomicMax(counters + CN_CHAIN, (ull)d);
  }
}

// ---- apply -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void apply_kernel(const int32_t* __restrict__ facet, const int32_t* __restrict__ newp,
                                                    int64_t npix, int32_t* __restrict__ roof)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= npix)
    return;
  const int32_t f = facet[i];
  if (f < 0)
    return;
  const int32_t p = newp[f];
  if (p > 0)
    roof[i] = p;
}

// ---- figures ---------------------------------------------------------------------------------------------------------
struct GenFig {  // device
  ull* b_changed;  // [n_buildings]
  ull* b_sum;
  ull* b_max;
  ull* p_in;  // [n_planes + 1]
  ull* p_out;
};

__device__ inline void plane_count(unsigned* s_tab, ull* g_tab, int32_t p, bool valid, ull m_valid)
{
  const int32_t p0 = __shfl(p, __ffsll((long long)m_valid) - 1);
  if (__all(!valid || p == p0)) {  // one plane over the whole wave: one add
    if ((threadIdx.x & 63) == 0) {
      if (p0 < BS_GEN_PLANE_CAP)
        atomicAdd(s_tab + p0, (unsigned)__popcll(m_valid));
      else
        atomicAdd(g_tab + p0, (ull)__popcll(m_valid));
    }
  } else if (valid) {
    if (p < BS_GEN_PLANE_CAP)
      atomicAdd(s_tab + p, 1u);
    else
      atomicAdd(g_tab + p, 1ull);
  }
}

__global__ __launch_bounds__(256) void gen_figures_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ roof0,
                                                          const int32_t* __restrict__ roof1, const int4* __restrict__ top0,
                                                          const int4* __restrict__ top1, int64_t npix, int32_t nb, int32_t npl,
                                                          GenFig G, ull* __restrict__ counters)
{
  __shared__ unsigned s_chg[BS_GEN_FIG_CAP];
  __shared__ ull s_sum[BS_GEN_FIG_CAP], s_max[BS_GEN_FIG_CAP];
  __shared__ unsigned s_pin[BS_GEN_PLANE_CAP], s_pout[BS_GEN_PLANE_CAP];
  __shared__ unsigned s_roofed;
  for (int k = threadIdx.x; k < BS_GEN_FIG_CAP; k += blockDim.x) {
    s_chg[k] = 0;
    s_sum[k] = s_max[k] = 0;
  }
  for (int k = threadIdx.x; k < BS_GEN_PLANE_CAP; k += blockDim.x)
    s_pin[k] = s_pout[k] = 0;
  if (threadIdx.x == 0)
    s_roofed = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t npix64 = (npix + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix64; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t c = -1, p0 = 0, p1 = 0;
    unsigned chg = 0;
    ull sum = 0, mx = 0;
    bool roofed = false;
    if (i < npix)
      c = map[i];
    if (c >= 0) {
      const int32_t r0 = roof0[i], r1 = roof1[i];
      p0 = r0 > 0 ? r0 : 0;
      p1 = r1 > 0 ? r1 : 0;
      chg = r0 != r1;
      roofed = p0 == 0 && p1 > 0;
      if (chg) {  // (the tops of a pixel depend on its own plane only)
        const int4 A = top0[i], B = top1[i];
        const long long d0 = (long long)B.x - A.x, d1 = (long long)B.y - A.y, d2 = (long long)B.z - A.z,
                        d3 = (long long)B.w - A.w;
        const ull a0 = (ull)(d0 < 0 ? -d0 : d0), a1 = (ull)(d1 < 0 ? -d1 : d1), a2 = (ull)(d2 < 0 ? -d2 : d2),
                  a3 = (ull)(d3 < 0 ? -d3 : d3);
        sum = a0 + a1 + a2 + a3;
        mx = max(max(a0, a1), max(a2, a3));
      }
    }
    const ull m_valid = __ballot(c >= 0);
    if (!m_valid)
      continue;
    const ull m_roofed = __ballot(roofed);
    if (lane == 0 && m_roofed)
      atomicAdd(&s_roofed, (unsigned)__popcll(m_roofed));
    plane_count(s_pin, G.p_in, p0, c >= 0, m_valid);
    plane_count(s_pout, G.p_out, p1, c >= 0, m_valid);
    if (!__ballot(chg != 0))
      continue;
    // runs of equal building inside the wave: one set of atomics per run
    const int32_t prev = __shfl_up(c, 1);
    const ull heads = __ballot(lane == 0 || prev != c);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    BS_SEG_SCAN(chg, BS_OP_ADD)
    BS_SEG_SCAN(sum, BS_OP_ADD)
    BS_SEG_SCAN(mx, BS_OP_MAX)
    if (lane == tl && c >= 0 && chg) {
      if (c < BS_GEN_FIG_CAP) {
        atomicAdd(s_chg + c, chg);
        atomicAdd(s_sum + c, sum);
        atomicMax(s_max + c, mx);
      } else {
        atomicAdd(G.b_changed + c, (ull)chg);
        atomicAdd(G.b_sum + c, sum);
        atomicMax(G.b_max + c, mx);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < BS_GEN_FIG_CAP && k < nb; k += blockDim.x)
    if (s_chg[k]) {
      atomicAdd(G.b_changed + k, (ull)s_chg[k]);
      atomicAdd(G.b_sum + k, s_sum[k]);
      atomicMax(G.b_max + k, s_max[k]);
    }
  for (int k = threadIdx.x; k < BS_GEN_PLANE_CAP && k <= npl; k += blockDim.x) {
    if (s_pin[k])
      atomicAdd(G.p_in + k, (ull)s_pin[k]);
    if (s_pout[k])
      atomicAdd(G.p_out + k, (ull)s_pout[k]);
  }
  if (threadIdx.x == 0 && s_roofed)
    atomicAdd(counters + CN_ROOFED, (ull)s_roofed);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct Eval {  // what one evaluation reports
  int64_t facets = 0, edges = 0, flat = 0, small = 0, movers = 0, movers_small = 0, movers_flat = 0, chain = 0;
  std::vector<ull> bfac;  // facets per building
};

struct Job {  // one call
  bs_ctx* ctx;
  const int32_t* map;  // the caller's
  int w, h;
  int32_t nb, npl, bin;
  Bases base;
  Tables tab;
  const int32_t* tab_flat;
  Rule rule;
  Events<8> ev;
  double ms_tops = 0, ms_facets = 0, ms_decide = 0;
};

// the two scans over the pixels that every evaluation runs; generalise_dev sizes their slot ahead, before the arrays exist
// (the rounds are launch-bound: every run here takes the slot as it was sized, cub_run_sized -- DESIGN.md)
auto number_scan(const int32_t* parent, int32_t* scan, int64_t npix, hipStream_t st)
{
  hipcub::TransformInputIterator<int32_t, RootFlag, hipcub::CountingInputIterator<int32_t>> roots(
      hipcub::CountingInputIterator<int32_t>(0), RootFlag{parent});
  return [=](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, roots, scan, (int)npix, st); };
}
auto border_scan(const uint8_t* flags, int32_t* scan, int64_t npix, hipStream_t st)
{
  return [=](void* tmp, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, FlagIt(flags, FlagCount()), scan, (int)npix, st);
  };
}

// One evaluation of the image in GN_ROOF: tops into `top`, facets and edges, the decision.  It leaves the facet image in
// GN_FACET and the new plane of every facet in GN_NEWP for the apply.
int evaluate(Job& J, int4* top, Eval* out)
{
  bs_ctx* ctx = J.ctx;
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->gn;
  const int w = J.w, h = J.h;
  const int64_t npix = (int64_t)w * h;
  const int ntx = nblk(w, LABEL_TW), nty = nblk(h, LABEL_TH);
  int32_t* roof = B[GN_ROOF].as<int32_t>();
  int32_t* cmap = B[GN_CMAP].as<int32_t>();
  int32_t* parent = B[GN_PARENT].as<int32_t>();
  int32_t* scan = B[GN_SCAN].as<int32_t>();
  uint8_t* flags = B[GN_FLAGS].as<uint8_t>();
  int32_t* facet = B[GN_FACET].as<int32_t>();
  ull* counters = B[GN_MISC].as<ull>();
  int* d_bad = reinterpret_cast<int*>(counters + CN_BAD);
  Events<8>& ev = J.ev;
  hipcub::CountingInputIterator<int32_t> idx(0);

  BS_HIP(ctx, hipMemsetAsync(counters, 0, 8 * CN_ROOFED, st));  // (CN_ROOFED belongs to the figures pass)
  if (J.nb > 0)
    BS_HIP(ctx, hipMemsetAsync(B[GN_BFAC].p, 0, 8 * (size_t)J.nb, st));
  // ---- 1. tops ----
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  tops_kernel<<<nblk(npix, 256), 256, 0, st>>>(J.map, roof, w, h, J.nb, J.npl, J.tab, J.tab_flat, J.bin, J.base, top, cmap,
                                               d_bad);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  // ---- 2. facets: label, number ----
  const Cls cls{cmap, roof};
  facet_tile_kernel<<<ntx * nty, 256, 0, st>>>(cls, w, h, ntx, J.nb, J.npl, parent, d_bad);
  {
    const int64_t n_h = (int64_t)(nty - 1) * w, total = n_h + (int64_t)(ntx - 1) * h;
    if (total > 0)
      facet_seam_kernel<<<nblk(total, 256), 256, 0, st>>>(cls, w, h, n_h, total, parent);
  }
  facet_flatten_kernel<<<nblk(npix, 256), 256, 0, st>>>(parent, npix);
  BS_HIP(ctx, cub_run_sized(B[GN_TMP], number_scan(parent, scan, npix, st)));
  int h_bad = 0;
  int32_t last_rank = 0, last_parent = -1;
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_rank, scan + npix - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_parent, parent + npix - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_bad)
    return fail(ctx, BS_ERR_RANGE,
                "roof generalise: a map value >= n_buildings, a roof value > n_planes, or a roof > 0 outside every building");
  const int64_t nf = (int64_t)last_rank + (last_parent == (int32_t)(npix - 1));
  out->facets = nf;
  out->bfac.assign((size_t)J.nb, 0);
  if (nf == 0) {  // no building pixel: nothing to decide
    BS_HIP(ctx, hipEventRecord(ev.e[2], st));
    BS_HIP(ctx, hipEventRecord(ev.e[3], st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    J.ms_tops += ev.ms(0, 1);
    J.ms_facets += ev.ms(1, 2);
    return BS_OK;
  }
  // ---- figures and border flags ----
  const size_t n = (size_t)nf;
  BS_HIP(ctx, B[GN_FFIG].reserve(FACET_FIG_BYTES * n));
  const FacetFig F = facet_fig_at(B[GN_FFIG].p, n);
  facet_fig_init_kernel<<<nblk(nf, 256), 256, 0, st>>>(F, nf);
  facet_write_kernel<<<nblk(npix, 256), 256, 0, st>>>(parent, scan, npix, facet);
  facet_figures_kernel<<<grid_of(npix), 256, 0, st>>>(cmap, roof, top, parent, facet, w, h, flags, F);
  BS_HIP(ctx, cub_run_sized(B[GN_TMP], border_scan(flags, scan, npix, st)));
  int32_t last_off = 0;
  uint8_t last_flag = 0;
  BS_HIP(ctx, hipMemcpyAsync(&last_off, scan + npix - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_flag, flags + npix - 1, 1, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  const int64_t nbord = (int64_t)last_off + (last_flag & 1) + (last_flag >> 1);
  // ---- edges ----
  int64_t ne = 0;
  EdgeFig E{};
  if (nbord > 0) {
    const int nbi = (int)nbord;
    const int end_bit = 32 + bits_of(nf);
    BS_HIP(ctx, B[GN_KEYS].reserve(8 * (size_t)nbord));
    BS_HIP(ctx, B[GN_KEYS2].reserve(8 * (size_t)nbord));
    BS_HIP(ctx, B[GN_VALS].reserve(4 * (size_t)nbord));
    BS_HIP(ctx, B[GN_VALS2].reserve(4 * (size_t)nbord));
    BS_HIP(ctx, B[GN_EID].reserve(4 * (size_t)nbord));
    ull* keys = B[GN_KEYS].as<ull>();
    ull* sorted = B[GN_KEYS2].as<ull>();
    int32_t* vals = B[GN_VALS].as<int32_t>();
    int32_t* svals = B[GN_VALS2].as<int32_t>();
    int32_t* eid = B[GN_EID].as<int32_t>();
    hipcub::TransformInputIterator<int32_t, HeadFlag, hipcub::CountingInputIterator<int32_t>> heads(idx, HeadFlag{sorted});
    auto sort = [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, sorted, vals, svals, nbi, 0, end_bit, st);
    };
    auto ids = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::InclusiveSum(tmp, bytes, heads, eid, nbi, st); };
    BS_HIP(ctx, cub_room(B[GN_TMP], sort, ids));
    edge_emit_kernel<<<grid_of(npix), 256, 0, st>>>(flags, scan, facet, w, npix, keys, vals);
    BS_HIP(ctx, cub_run_sized(B[GN_TMP], sort));
    BS_HIP(ctx, cub_run_sized(B[GN_TMP], ids));
    int32_t h_ne = 0;
    BS_HIP(ctx, hipMemcpyAsync(&h_ne, eid + nbord - 1, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    BS_HIP(ctx, hipGetLastError());
    ne = h_ne;
    BS_HIP(ctx, B[GN_EFIG].reserve(EDGE_FIG_BYTES * (size_t)ne));
    E = edge_fig_at(B[GN_EFIG].p, (size_t)ne);
    edge_fig_init_kernel<<<nblk(ne, 256), 256, 0, st>>>(E, ne);
    edge_reduce_kernel<<<grid_of(nbord), 256, 0, st>>>(sorted, svals, eid, nbord, cmap, top, facet, w, E);
  }
  out->edges = ne;
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  // ---- 3 to 8. decide ----
  BS_HIP(ctx, B[GN_RKEY].reserve(8 * n));
  BS_HIP(ctx, B[GN_RKEY2].reserve(8 * n));
  BS_HIP(ctx, B[GN_ORDER].reserve(4 * n));
  BS_HIP(ctx, B[GN_BEST].reserve(8 * n));
  BS_HIP(ctx, B[GN_NEXT].reserve(4 * n));
  BS_HIP(ctx, B[GN_NEXT2].reserve(4 * n));
  BS_HIP(ctx, B[GN_DIST].reserve(4 * n));
  BS_HIP(ctx, B[GN_DIST2].reserve(4 * n));
  BS_HIP(ctx, B[GN_NEWP].reserve(4 * n));
  ull* rkey = B[GN_RKEY].as<ull>();
  ull* rsorted = B[GN_RKEY2].as<ull>();
  int32_t* order = B[GN_ORDER].as<int32_t>();
  ull* best = B[GN_BEST].as<ull>();
  int32_t* next = B[GN_NEXT].as<int32_t>();
  int32_t* next2 = B[GN_NEXT2].as<int32_t>();
  int32_t* dist = B[GN_DIST].as<int32_t>();
  int32_t* dist2 = B[GN_DIST2].as<int32_t>();
  auto rank = [&](void* tmp, size_t& bytes) { return hipcub::DeviceRadixSort::SortKeys(tmp, bytes, rkey, rsorted, (int)nf, 0, 63, st); };
  BS_HIP(ctx, cub_room(B[GN_TMP], rank));
  rank_key_kernel<<<nblk(nf, 256), 256, 0, st>>>(F.pixels, nf, rkey);
  BS_HIP(ctx, cub_run_sized(B[GN_TMP], rank));
  order_kernel<<<nblk(nf, 256), 256, 0, st>>>(rsorted, nf, order, best);
  if (ne > 0)
    candidates_kernel<<<grid_of(ne), 256, 0, st>>>(E, ne, F.pixels, F.plane, order, J.rule, best, counters);
  resolve_kernel<<<grid_of(nf), 256, 0, st>>>(nf, best, rsorted, F.pixels, F.building, J.rule.min_pixels, next, dist, counters,
                                              B[GN_BFAC].as<ull>());
  for (int k = bits_of(nf); k > 0; k--) {  // 2^bits_of(nf) >= nf > the links of any chain
    double_kernel<<<nblk(nf, 256), 256, 0, st>>>(nf, next, dist, next2, dist2);
    std::swap(next, next2);
    std::swap(dist, dist2);
  }
  new_plane_kernel<<<grid_of(nf), 256, 0, st>>>(nf, next, dist, F.plane, B[GN_NEWP].as<int32_t>(), counters);
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  ull hc[CN_COUNT] = {};
  BS_HIP(ctx, hipMemcpyAsync(hc, counters, sizeof hc, hipMemcpyDeviceToHost, st));
  if (J.nb > 0)
    BS_HIP(ctx, hipMemcpyAsync(out->bfac.data(), B[GN_BFAC].p, 8 * (size_t)J.nb, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  out->flat = (int64_t)hc[CN_FLAT];
  out->small = (int64_t)hc[CN_SMALL];
  out->movers = (int64_t)hc[CN_MOVERS];
  out->movers_small = (int64_t)hc[CN_MOVERS_SMALL];
  out->movers_flat = (int64_t)hc[CN_MOVERS_FLAT];
  out->chain = (int64_t)hc[CN_CHAIN];
  J.ms_tops += ev.ms(0, 1);
  J.ms_facets += ev.ms(1, 2);
  J.ms_decide += ev.ms(2, 3);
  return BS_OK;
}

template <class T>
T* host_copy(const std::vector<T>& v)
{
  T* p = (T*)calloc(std::max<size_t>(v.size(), 1), sizeof(T));
  if (p && !v.empty())
    memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

const char* const GEN_INVALID =
    "roof generalise: null pointer, width or height < 1, width * height >= 2^30, n_buildings or n_planes < 0, bin < 1, or a "
    "negative parameter";

bool bad_call(int32_t w, int32_t h, int32_t nb, int32_t npl, const double* normal, const int32_t* center, const int32_t* z_min,
              const int32_t* z_max, int32_t bin, const int32_t* flat, const struct bs_roof_generalise_params* p)
{
  return w < 1 || h < 1 || (int64_t)w * h >= (1ll << 30) || ((int64_t)w + 1) * ((int64_t)h + 1) >= (1ll << 31) || nb < 0 ||
         npl < 0 || bin < 1 || (nb > 0 && !flat) || (npl > 0 && (!normal || !center || !z_min || !z_max)) || !p ||
         p->min_pixels < 0 || p->merge_flat < 0 || p->step_tol < 0 || p->bend_tol < 0 || p->max_rounds < 0;
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_roof_generalise_free(struct bs_roof_generalise* g)
{
  if (!g)
    return;
  free(g->eval_facets);
  free(g->eval_movers);
  free(g->eval_movers_small);
  free(g->eval_movers_flat);
  free(g->eval_longest_chain);
  free(g->plane_pixels_in);
  free(g->plane_pixels_out);
  free(g->building_facets_in);
  free(g->building_facets_out);
  free(g->building_pixels_changed);
  free(g->building_sum_abs_dtop);
  free(g->building_max_abs_dtop);
  memset(g, 0, sizeof *g);
}

extern "C" int bs_roof_generalise_dev(bs_ctx* ctx, const int32_t* d_map, const int32_t* d_roof, int32_t width, int32_t height,
                                      int32_t n_buildings, int32_t n_planes, const double* normal, const int32_t* center,
                                      const int32_t* z_min, const int32_t* z_max, int32_t bin, int32_t base_z,
                                      const int32_t* flat, const struct bs_roof_generalise_params* params,
                                      int32_t* d_roof_out, struct bs_roof_generalise* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_map || !d_roof || !d_roof_out || !out ||
      bad_call(width, height, n_buildings, n_planes, normal, center, z_min, z_max, bin, flat, params))
    return fail(ctx, BS_ERR_INVALID, GEN_INVALID);
  const int32_t* d_bases = nullptr;
  if (const int rc = building_bases(ctx, n_buildings, "roof generalisation", &d_bases))
    return rc;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int w = width, h = height;
  const int32_t nb = n_buildings, npl = n_planes;
  const int64_t npix = (int64_t)w * h;
  const size_t mp = (size_t)std::max(npl, 1), mb = (size_t)std::max(nb, 1);
  DevBuf* B = ctx->gn;
  Job J;
  J.ctx = ctx;
  J.map = d_map;
  J.w = w;
  J.h = h;
  J.nb = nb;
  J.npl = npl;
  J.bin = bin;
  J.base = Bases{d_bases, base_z};
  J.rule = Rule{(long long)params->min_pixels, params->merge_flat != 0, params->step_tol, params->bend_tol};
  for (auto& e : J.ev.e)
    BS_HIP(ctx, hipEventCreate(&e));

  BS_HIP(ctx, B[GN_ROOF].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[GN_CMAP].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[GN_TOP0].reserve(16 * (size_t)npix));
  BS_HIP(ctx, B[GN_TOP1].reserve(16 * (size_t)npix));
  BS_HIP(ctx, B[GN_PARENT].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[GN_SCAN].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[GN_FLAGS].reserve((size_t)npix));
  BS_HIP(ctx, B[GN_FACET].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[GN_MISC].reserve(8 * CN_COUNT));
  BS_HIP(ctx, B[GN_TAB].reserve(44 * mp + 4 * mb));
  BS_HIP(ctx, B[GN_BFAC].reserve(8 * mb));
  BS_HIP(ctx, B[GN_FIG].reserve(24 * mb + 16 * (mp + 1)));
  BS_HIP(ctx, cub_room(B[GN_TMP], number_scan(nullptr, nullptr, npix, st), border_scan(nullptr, nullptr, npix, st)));
  double* tab_normal = B[GN_TAB].as<double>();
  int32_t* tab_center = reinterpret_cast<int32_t*>(tab_normal + 3 * mp);
  int32_t* tab_zmin = tab_center + 3 * mp;
  int32_t* tab_zmax = tab_zmin + mp;
  int32_t* tab_flat = tab_zmax + mp;
  J.tab = Tables{tab_normal, tab_center, tab_zmin, tab_zmax};
  J.tab_flat = tab_flat;
  if (npl > 0) {
    BS_HIP(ctx, hipMemcpyAsync(tab_normal, normal, 24 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_center, center, 12 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_zmin, z_min, 4 * (size_t)npl, hipMemcpyHostToDevice, st));
    BS_HIP(ctx, hipMemcpyAsync(tab_zmax, z_max, 4 * (size_t)npl, hipMemcpyHostToDevice, st));
  }
  if (nb > 0)
    BS_HIP(ctx, hipMemcpyAsync(tab_flat, flat, 4 * (size_t)nb, hipMemcpyHostToDevice, st));
  int32_t* roof = B[GN_ROOF].as<int32_t>();
  BS_HIP(ctx, hipMemcpyAsync(roof, d_roof, 4 * (size_t)npix, hipMemcpyDeviceToDevice, st));
  // ---- the rounds ----
  std::vector<int64_t> e_facets, e_movers, e_small, e_flat, e_chain;
  Eval first, last;
  int4* top0 = B[GN_TOP0].as<int4>();
  int4* top_last = top0;
  int32_t rounds = 0, converged = 0;
  double ms_apply = 0;
  for (int32_t r = 1;; r++) {
    Eval cur;
    top_last = r == 1 ? top0 : B[GN_TOP1].as<int4>();
    const int rc = evaluate(J, top_last, &cur);
    if (rc != BS_OK)
      return rc;
    e_facets.push_back(cur.facets);
    e_movers.push_back(cur.movers);
    e_small.push_back(cur.movers_small);
    e_flat.push_back(cur.movers_flat);
    e_chain.push_back(cur.chain);
    if (r == 1)
      first = cur;
    last = std::move(cur);
    if (last.movers == 0) {
      converged = 1;
      break;
    }
    if (r > params->max_rounds)
      break;
    BS_HIP(ctx, hipEventRecord(J.ev.e[4], st));
    apply_kernel<<<nblk(npix, 256), 256, 0, st>>>(B[GN_FACET].as<int32_t>(), B[GN_NEWP].as<int32_t>(), npix, roof);
    BS_HIP(ctx, hipEventRecord(J.ev.e[5], st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    ms_apply += J.ev.ms(4, 5);
    rounds = r;
  }

  // ---- figures: the input against the result, the first tops against the last ----
  GenFig G;
  G.b_changed = B[GN_FIG].as<ull>();
  G.b_sum = G.b_changed + mb;
  G.b_max = G.b_sum + mb;
  G.p_in = G.b_max + mb;
  G.p_out = G.p_in + (mp + 1);
  ull* counters = B[GN_MISC].as<ull>();
  BS_HIP(ctx, hipMemsetAsync(B[GN_FIG].p, 0, 24 * mb + 16 * (mp + 1), st));
  BS_HIP(ctx, hipMemsetAsync(counters + CN_ROOFED, 0, 8, st));
  BS_HIP(ctx, hipEventRecord(J.ev.e[6], st));
  gen_figures_kernel<<<grid_of(npix), 256, 0, st>>>(B[GN_CMAP].as<int32_t>(), d_roof, roof, top0, top_last, npix, nb, npl, G,
                                                    counters);
  BS_HIP(ctx, hipEventRecord(J.ev.e[7], st));
  std::vector<ull> hb(3 * mb), hp(2 * (mp + 1));
  ull h_roofed = 0;
  BS_HIP(ctx, hipMemcpyAsync(hb.data(), G.b_changed, 24 * mb, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(hp.data(), G.p_in, 16 * (mp + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&h_roofed, counters + CN_ROOFED, 8, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());

  struct bs_roof_generalise res;
  memset(&res, 0, sizeof res);
  const size_t np1 = (size_t)npl + 1, nbs = (size_t)nb;
  std::vector<int64_t> v_pin(np1), v_pout(np1), v_fin(nbs), v_fout(nbs), v_chg(nbs), v_sum(nbs), v_max(nbs);
  int64_t changed = 0;
  for (size_t p = 0; p < np1; p++) {
    v_pin[p] = (int64_t)hp[p];
    v_pout[p] = (int64_t)hp[mp + 1 + p];
  }
  for (size_t c = 0; c < nbs; c++) {
    v_fin[c] = (int64_t)first.bfac[c];
    v_fout[c] = (int64_t)last.bfac[c];
    v_chg[c] = (int64_t)hb[c];
    v_sum[c] = (int64_t)hb[mb + c];
    v_max[c] = (int64_t)hb[2 * mb + c];
    changed += v_chg[c];
  }
  res.eval_facets = host_copy(e_facets);
  res.eval_movers = host_copy(e_movers);
  res.eval_movers_small = host_copy(e_small);
  res.eval_movers_flat = host_copy(e_flat);
  res.eval_longest_chain = host_copy(e_chain);
  res.plane_pixels_in = host_copy(v_pin);
  res.plane_pixels_out = host_copy(v_pout);
  res.building_facets_in = host_copy(v_fin);
  res.building_facets_out = host_copy(v_fout);
  res.building_pixels_changed = host_copy(v_chg);
  res.building_sum_abs_dtop = host_copy(v_sum);
  res.building_max_abs_dtop = host_copy(v_max);
  if (!res.eval_facets || !res.eval_movers || !res.eval_movers_small || !res.eval_movers_flat || !res.eval_longest_chain ||
      !res.plane_pixels_in || !res.plane_pixels_out || !res.building_facets_in || !res.building_facets_out ||
      !res.building_pixels_changed || !res.building_sum_abs_dtop || !res.building_max_abs_dtop) {
    bs_roof_generalise_free(&res);
    return fail(ctx, BS_ERR_NOMEM, "roof generalise: host allocation");
  }
  // ---- everything has succeeded: the result leaves the scratch ----
  {
    hipError_t e = hipMemcpyAsync(d_roof_out, roof, 4 * (size_t)npix, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess)
      e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      bs_roof_generalise_free(&res);
      return fail(ctx, BS_ERR_HIP, "roof generalise: copy of the result", e);
    }
  }
  res.width = w;
  res.height = h;
  res.n_buildings = nb;
  res.n_planes = npl;
  res.rounds = rounds;
  res.converged = converged;
  res.n_facets_in = first.facets;
  res.n_facets_out = last.facets;
  res.n_edges_in = first.edges;
  res.n_edges_out = last.edges;
  res.n_flat_in = first.flat;
  res.n_flat_out = last.flat;
  res.n_small_in = first.small;
  res.n_small_out = last.small;
  res.pixels_changed = changed;
  res.pixels_roofed = (int64_t)h_roofed;
  res.ms_tops = J.ms_tops;
  res.ms_facets = J.ms_facets;
  res.ms_decide = J.ms_decide;
  res.ms_apply = ms_apply;
  res.ms_figures = J.ev.ms(6, 7);
  *out = res;
  return BS_OK;
}

extern "C" int bs_roof_generalise(bs_ctx* ctx, const int32_t* map, const int32_t* roof, int32_t width, int32_t height,
                                  int32_t n_buildings, int32_t n_planes, const double* normal, const int32_t* center,
                                  const int32_t* z_min, const int32_t* z_max, int32_t bin, int32_t base_z, const int32_t* flat,
                                  const struct bs_roof_generalise_params* params, int32_t* roof_out,
                                  struct bs_roof_generalise* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!map || !roof || !roof_out || !out ||
      bad_call(width, height, n_buildings, n_planes, normal, center, z_min, z_max, bin, flat, params))
    return fail(ctx, BS_ERR_INVALID, GEN_INVALID);
  const size_t npix = (size_t)width * height;
  DevBuf* B = ctx->gn;
  Staging S(ctx);
  int32_t* d_out = S.room<int32_t>(B[GN_OUT], npix);
  const int32_t* d_roof = S.upload(B[GN_IN_ROOF], roof, npix);
  const int32_t* d_map = S.upload(B[GN_IN_MAP], map, npix);
  if (!S.ok())
    return S.status();
  struct bs_roof_generalise res;
  int rc = bs_roof_generalise_dev(ctx, d_map, d_roof, width, height, n_buildings, n_planes, normal, center, z_min, z_max, bin,
                                  base_z, flat, params, d_out, &res);
  if (rc != BS_OK)
    return rc;
  FreeUnlessKept<struct bs_roof_generalise, bs_roof_generalise_free> guard{&res};
  S.download(roof_out, d_out, npix);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  *out = res;
  return BS_OK;
}
