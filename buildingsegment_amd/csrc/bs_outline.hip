// bs_outline.hip -- the outline of every label of a label image as polygon rings with holes (DESIGN.md "Facet outlines";
// the definition is written down in include/bs_api.h under "facet outlines").
//   half-edges  one pixel pass: the four side flags of a pixel and their popcount in one byte, and the range check; a wave
//               without a labelled pixel does one load and one store.  One exclusive sum of the popcounts = base[pixel]; the
//               compact id of side k of pixel p is base[p] + popcount(flags[p] & ((1 << k) - 1)): ascending half-edge
//               number.  Successor, vertex flag and Z per compact half-edge from the rules of the header.
//   leaders     the lowest id of every cycle by pointer doubling: R = ceil(log2 n_half) rounds, double-buffered
//   rank        the cycle cut in front of its leader, then R Wyllie rounds that carry the number of vertex half-edges
//               from each element to the tail: a vertex stands at (vertices of its ring) - (its suffix count)
//   rings       leaders flagged and scanned (= a slot per ring), the order-free figures reduced over runs of equal ring
//               inside a wave before one set of atomics per run, the slots sorted by (label << 32) | leader, the vertex
//               counts scanned, the first ring of every label by binary search, the place of every vertex
//   emit        a vertex half-edge stores its corner and its Z at its place
// No thread walks a ring: every round count comes from the host, the only loops in kernels are grid strides, the four
// sides of a pixel, the six steps of a wave scan and a binary search of host-given depth.  Every index read from memory
// is checked before it is used as an address; a violation sets err and the call returns BS_ERR_INTERNAL.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bs_chain.h"  // (bad_image)
#include "bs_common.h"
#include "bs_host.h"
#include "bs_outline.h"
#include "bs_segscan.h"

namespace bs {
namespace {

// ---- half-edges ----------------------------------------------------------------------------------------------------------
// flags[pixel]: bit k = side k is a half-edge (k = 0 north, 1 east, 2 south, 3 west: the neighbour p + delta[k] is outside
// the image or of another label), bits 4..6 their popcount
__global__ __launch_bounds__(256) void outline_flags_kernel(const int32_t* __restrict__ label, int w, int h, int32_t n_labels,
                                                            uint8_t* __restrict__ flags, int* __restrict__ bad)
{
  const int64_t npix = (int64_t)w * h;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = label[i];
    unsigned f = 0;
    if (l >= 0) {  // (a wave without a labelled pixel branches around the neighbour loads as a whole)
      if (l >= n_labels)
        atomicOr(bad, 1);
      const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
      f = (unsigned)(y == 0 || label[i - w] != l) | ((unsigned)(x + 1 >= w || label[i + 1] != l) << 1) |
          ((unsigned)(y + 1 >= h || label[i + w] != l) << 2) | ((unsigned)(x == 0 || label[i - 1] != l) << 3);
      f |= (unsigned)__popc(f) << 4;
    }
    flags[i] = (uint8_t)f;
  }
}

struct SideCount {
  __host__ __device__ int32_t operator()(uint8_t v) const { return v >> 4; }
};
using SideIt = hipcub::TransformInputIterator<int32_t, SideCount, const uint8_t*>;

// the number 4 * pixel + side of every compact half-edge
__global__ __launch_bounds__(256) void outline_compact_kernel(const uint8_t* __restrict__ flags, const int32_t* __restrict__ base,
                                                              int64_t npix, int32_t n, int32_t* __restrict__ hnum,
                                                              int* __restrict__ err)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned f = flags[i];
    if (!(f & 15u))
      continue;
    int32_t at = base[i];
    for (int k = 0; k < 4; k++) {
      if (!((f >> k) & 1u))
        continue;
      if ((uint32_t)at < (uint32_t)n)
        hnum[at] = (int32_t)(4 * i + k);
      else
        atomicOr(err, 1);
      at++;
    }
  }
}

struct Image {
  const int32_t* label;
  int w, h;
  // in(r, p): r is inside the image and has the label l of p
  __device__ bool in(int x, int y, int32_t l) const { return x >= 0 && x < w && y >= 0 && y < h && label[(int64_t)y * w + x] == l; }
};

__device__ inline int dx_of(int k) { return (k == 1) - (k == 3); }
__device__ inline int dy_of(int k) { return (k == 2) - (k == 0); }

// successor, vertex flag and Z of every compact half-edge: the label reads are the pixel itself, q and b
__global__ __launch_bounds__(256) void outline_succ_kernel(Image im, const int32_t* __restrict__ top,
                                                           const uint8_t* __restrict__ flags, const int32_t* __restrict__ base,
                                                           const int32_t* __restrict__ hnum, int32_t n, int32_t* __restrict__ succ,
                                                           uint8_t* __restrict__ vert, int32_t* __restrict__ zv,
                                                           int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t hn = hnum[i];
  const int64_t p = hn >> 2, npix = (int64_t)im.w * im.h;
  const int k = hn & 3, k1 = (k + 1) & 3, k3 = (k + 3) & 3;
  if (hn < 0 || p >= npix) {
    atomicOr(err, 2);
    succ[i] = (int32_t)i;
    vert[i] = 0;
    return;
  }
  const int y = (int)(p / im.w), x = (int)(p - (int64_t)y * im.w);
  const int32_t l = im.label[p];
  const unsigned f = flags[p];
  int tx = x, ty = y, tk = k1;  // a left turn stays on the pixel
  if (!((f >> k1) & 1u)) {      // (the side k1 is no half-edge: p' is inside and of this label)
    const int px = x + dx_of(k1), py = y + dy_of(k1);
    const int qx = px + dx_of(k), qy = py + dy_of(k);
    if (!im.in(qx, qy, l)) {
      tx = px, ty = py, tk = k;  // straight on
    } else {
      tx = qx, ty = qy, tk = k3;  // a right turn
    }
  }
  const bool inside = tx >= 0 && tx < im.w && ty >= 0 && ty < im.h;  // (it is, unless flags and label disagree)
  const int64_t tp = inside ? (int64_t)ty * im.w + tx : p;
  const unsigned tf = flags[tp];
  const int32_t s = base[tp] + __popc(tf & ((1u << tk) - 1u));
  if (!inside || !((tf >> tk) & 1u) || (uint32_t)s >= (uint32_t)n) {
    atomicOr(err, 2);
    succ[i] = (int32_t)i;
  } else {
    succ[i] = s;
  }
  // a vertex iff the predecessor has another side number
  const bool v = ((f >> k3) & 1u) || im.in(x + dx_of(k3) + dx_of(k), y + dy_of(k3) + dy_of(k), l);
  vert[i] = v;
  if (top && v)
    zv[i] = top[4 * p + (k ^ (k >> 1))];  // the start corner of side k: t00, t10, t11, t01
}

// ---- leaders -------------------------------------------------------------------------------------------------------------
// one doubling round: mn = the lowest id among the 2^round elements from here on (mn == nullptr: the identity)
__global__ __launch_bounds__(256) void outline_min_kernel(const int32_t* __restrict__ mn, const int32_t* __restrict__ nxt,
                                                          int32_t n, int32_t* __restrict__ mn2, int32_t* __restrict__ nxt2,
                                                          int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  int32_t j = nxt[i];
  if ((uint32_t)j >= (uint32_t)n) {
    atomicOr(err, 4);
    j = (int32_t)i;
  }
  const int32_t a = mn ? mn[i] : (int32_t)i, b = mn ? mn[j] : j;
  mn2[i] = min(a, b);
  nxt2[i] = nxt[j];
}

// ---- rings ---------------------------------------------------------------------------------------------------------------
struct LeadFlag {  // a half-edge that is the lowest of its ring
  const int32_t* leader;
  __host__ __device__ int32_t operator()(int32_t i) const { return leader[i] == i; }
};

struct SlotFig {  // per ring slot (ascending leader), device
  unsigned long long* length;
  unsigned long long* area2;  // (two's complement sum)
  int32_t* bbox;
  int32_t* vertices;
  int32_t* start;
};
constexpr size_t SLOT_FIG_BYTES = 2 * 8 + 6 * 4;

SlotFig slot_fig_at(void* p, size_t n)
{
  SlotFig f;
  f.length = (unsigned long long*)p;
  f.area2 = f.length + n;
  f.bbox = (int32_t*)(f.area2 + n);
  f.vertices = f.bbox + 4 * n;
  f.start = f.vertices + n;
  return f;
}

__global__ __launch_bounds__(256) void outline_slot_init_kernel(SlotFig F, int32_t nr)
{
  const int64_t s = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (s >= nr)
    return;
  F.length[s] = F.area2[s] = 0;
  F.bbox[4 * s] = F.bbox[4 * s + 1] = INT32_MAX;
  F.bbox[4 * s + 2] = F.bbox[4 * s + 3] = INT32_MIN;
  F.vertices[s] = F.start[s] = 0;
}

// One lane per half-edge.  A leader names its ring: key, vertex count, start.  Length, area and box are reduced over the
// runs of equal slot inside the wave (neighbouring compact ids lie on one ring along every straight run of a border):
// with one set of atomics per half-edge instead, the rings phase took 3.7 times as long at bin 25.
__global__ __launch_bounds__(256) void outline_figures_kernel(const int32_t* __restrict__ hnum, const int32_t* __restrict__ leader,
                                                              const int32_t* __restrict__ slot, const int32_t* __restrict__ val,
                                                              const int32_t* __restrict__ label, int w, int32_t n, int32_t nr,
                                                              unsigned long long* __restrict__ keys, int32_t* __restrict__ vals,
                                                              SlotFig F, int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int64_t n64 = ((int64_t)n + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n64; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t s = -1;
    long long area = 0;
    int X0 = INT32_MAX, Y0 = INT32_MAX, X1 = INT32_MIN, Y1 = INT32_MIN;
    if (i < n) {
      const int32_t L = leader[i];
      if ((uint32_t)L < (uint32_t)n)
        s = slot[L];
      if ((uint32_t)s >= (uint32_t)nr) {
        atomicOr(err, 16);
        s = -1;
      } else {
        const int32_t hn = hnum[i];
        const int64_t p = hn >> 2;
        const int k = hn & 3, k1 = (k + 1) & 3;
        const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
        const int sx = x + (k == 1 || k == 2), sy = y + (k >= 2), ex = x + (k1 == 1 || k1 == 2), ey = y + (k1 >= 2);
        area = (long long)sx * ey - (long long)ex * sy;
        X0 = min(sx, ex), Y0 = min(sy, ey), X1 = max(sx, ex), Y1 = max(sy, ey);
        if (L == (int32_t)i) {
          keys[s] = ((unsigned long long)(uint32_t)label[p] << 32) | (uint32_t)L;
          vals[s] = s;
          F.vertices[s] = val[i];
          F.start[s] = hn;
        }
      }
    }
    const int32_t prev = __shfl_up(s, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != s);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    BS_SEG_SCAN(area, BS_OP_ADD)
    BS_SEG_SCAN(X0, BS_OP_MIN)
    BS_SEG_SCAN(Y0, BS_OP_MIN)
    BS_SEG_SCAN(X1, BS_OP_MAX)
    BS_SEG_SCAN(Y1, BS_OP_MAX)
    if (lane == tl && s >= 0) {
      atomicAdd(F.length + s, (unsigned long long)(tl - hl + 1));
      atomicAdd(F.area2 + s, (unsigned long long)area);
      atomicMin(F.bbox + 4 * (int64_t)s, X0);
      atomicMin(F.bbox + 4 * (int64_t)s + 1, Y0);
      atomicMax(F.bbox + 4 * (int64_t)s + 2, X1);
      atomicMax(F.bbox + 4 * (int64_t)s + 3, Y1);
    }
  }
}

// the rings in the listed order from the sorted (key, slot) pairs
__global__ __launch_bounds__(256) void outline_gather_kernel(const unsigned long long* __restrict__ skeys,
                                                             const int32_t* __restrict__ svals, int32_t nr, SlotFig F, RingOut R,
                                                             int* __restrict__ err)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nr)
    return;
  const int32_t s = svals[r];
  if ((uint32_t)s >= (uint32_t)nr) {
    atomicOr(err, 32);
    return;
  }
  R.of_slot[s] = (int32_t)r;
  R.label[r] = (int32_t)(skeys[r] >> 32);
  R.start[r] = F.start[s];
  R.vertices[r] = F.vertices[s];
  R.length[r] = F.length[s];
  R.area2[r] = F.area2[s];
  for (int c = 0; c < 4; c++)
    R.bbox[4 * r + c] = F.bbox[4 * (int64_t)s + c];
}

struct VertexCount {  // the vertex count of ring r, 0 for the entry behind the last
  const int32_t* vertices;
  int32_t nr;
  __host__ __device__ int32_t operator()(int32_t r) const { return r < nr ? vertices[r] : 0; }
};

// label_ring_offset[l] = the first ring whose label is >= l: a binary search of `steps` halvings (from the host)
__global__ __launch_bounds__(256) void outline_label_offset_kernel(const int32_t* __restrict__ ring_label, int32_t nr,
                                                                   int32_t n_labels, int steps, int32_t* __restrict__ lro)
{
  const int64_t l = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (l > n_labels)
    return;
  int32_t lo = 0, hi = nr;  // the answer lies in [lo, hi]
  for (int s = 0; s < steps; s++) {
    if (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (ring_label[mid] < l)
        lo = mid + 1;
      else
        hi = mid;
    }
  }
  lro[l] = lo;
}

// the place of every vertex half-edge in the vertex arrays, -1 for the others
__global__ __launch_bounds__(256) void outline_place_kernel(const uint8_t* __restrict__ vert, const int32_t* __restrict__ leader,
                                                            const int32_t* __restrict__ slot, const int32_t* __restrict__ val,
                                                            const int32_t* __restrict__ nxt, int32_t n, int32_t nr, RingOut R,
                                                            int32_t* __restrict__ dest, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  int32_t d = -1;
  if (nxt[i] != END)
    atomicOr(err, 64);  // the list did not close within the rounds
  if (vert[i]) {
    const int32_t L = leader[i];
    const int32_t s = (uint32_t)L < (uint32_t)n ? slot[L] : -1;
    const int32_t r = (uint32_t)s < (uint32_t)nr ? R.of_slot[s] : -1;
    if ((uint32_t)r >= (uint32_t)nr) {
      atomicOr(err, 64);
    } else {
      const int32_t nv = R.vertices[r], pos = nv - val[i];
      if (pos < 0 || pos >= nv)
        atomicOr(err, 64);
      else
        d = R.offset[r] + pos;
    }
  }
  dest[i] = d;
}

// ---- emit ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void outline_emit_kernel(const int32_t* __restrict__ hnum, const int32_t* __restrict__ dest,
                                                           const int32_t* __restrict__ zv, int w, int32_t n, int32_t nv,
                                                           int2* __restrict__ xy, int32_t* __restrict__ z, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t d = dest[i];
  if (d < 0)
    return;
  if (d >= nv) {
    atomicOr(err, 128);
    return;
  }
  const int32_t hn = hnum[i];
  const int64_t p = hn >> 2;
  const int k = hn & 3;
  const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
  xy[d] = make_int2(x + (k == 1 || k == 2), y + (k >= 2));
  if (z)
    z[d] = zv[i];
}

using Guard = FreeUnlessKept<struct bs_outlines, bs_outlines_free>;

const char* const OUTLINES_INVALID = "facet outlines: null pointer, width or height < 1, width * height >= 2^29, n_labels < 0, "
                                     "or d_top not 16-byte aligned";

int internal(bs_ctx* ctx, int err)
{
  char msg[96];
  snprintf(msg, sizeof msg, "facet outlines: an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_outlines_free(struct bs_outlines* s)
{
  if (!s)
    return;
  free(s->ring_label);
  free(s->ring_start);
  free(s->ring_length);
  free(s->ring_vertices);
  free(s->ring_area2);
  free(s->ring_bbox);
  free(s->ring_offset);
  free(s->label_ring_offset);
  free(s->xy);
  free(s->z);
  memset(s, 0, sizeof *s);
}

extern "C" int bs_facet_outlines_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width,
                                           int32_t height, int32_t n_labels, struct bs_outlines* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->ol_valid = false;
  if (!d_label || !out || bad_image(width, height) || n_labels < 0 || (reinterpret_cast<uintptr_t>(d_top) & 15u))
    return fail(ctx, BS_ERR_INVALID, OUTLINES_INVALID);
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int w = width, h = height;
  const int64_t npix = (int64_t)w * h;
  DevBuf* B = ctx->ol;
  Events<10> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));
  hipcub::CountingInputIterator<int32_t> idx(0);

  struct bs_outlines res;
  memset(&res, 0, sizeof res);
  Guard guard{&res};
  res.width = w;
  res.height = h;
  res.n_labels = n_labels;
  res.has_z = d_top != nullptr;
  if (!alloc(&res.label_ring_offset, (size_t)n_labels + 1))
    return fail(ctx, BS_ERR_NOMEM, "facet outlines: host allocation");

  // ---- half-edges: flags and base ----
  BS_HIP(ctx, B[OL_FLAGS].reserve((size_t)npix));
  BS_HIP(ctx, B[OL_BASE].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[OL_MISC].reserve(256));
  uint8_t* flags = B[OL_FLAGS].as<uint8_t>();
  int32_t* base = B[OL_BASE].as<int32_t>();
  int* d_bad = B[OL_MISC].as<int>();
  int* d_err = d_bad + 1;
  auto sides = [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, SideIt(flags, SideCount()), base, (int)npix, st);
  };
  BS_HIP(ctx, cub_room(B[OL_TMP], sides));
  BS_HIP(ctx, hipMemsetAsync(d_bad, 0, 8, st));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  outline_flags_kernel<<<grid_of(npix), 256, 0, st>>>(d_label, w, h, n_labels, flags, d_bad);
  BS_HIP(ctx, cub_run_sized(B[OL_TMP], sides));
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  int h_bad = 0;
  int32_t last_base = 0;
  uint8_t last_flag = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_base, base + npix - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_flag, flags + npix - 1, 1, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // round trip 1: n_half
  BS_HIP(ctx, hipGetLastError());
  if (h_bad)
    return fail(ctx, BS_ERR_RANGE, "facet outlines: a label >= n_labels");
  const int64_t n_half = (int64_t)last_base + (last_flag >> 4);
  res.ms_halfedges = ev.ms(0, 1);
  if (n_half == 0) {  // no labelled pixel: no ring, every offset 0
    if (!alloc(&res.ring_offset, 1))
      return fail(ctx, BS_ERR_NOMEM, "facet outlines: host allocation");
    ctx->ol_nhalf = ctx->ol_nv = 0;
    ctx->ol_has_z = d_top != nullptr;
    ctx->ol_valid = true;
    *out = res;
    guard.keep = true;
    return BS_OK;
  }
  const int32_t n = (int32_t)n_half;  // (< 2^31: the check on the image)
  const int R = rounds_of(n_half);

  // ---- half-edges: numbers, successors, vertex flags ----
  for (int b : {OL_HNUM, OL_SUCC, OL_MN0, OL_MN1, OL_NX0, OL_NX1, OL_VAL0, OL_VAL1, OL_ZV, OL_DEST, OL_SLOT})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)n));
  BS_HIP(ctx, B[OL_VERT].reserve((size_t)n));
  int32_t* hnum = B[OL_HNUM].as<int32_t>();
  int32_t* succ = B[OL_SUCC].as<int32_t>();
  uint8_t* vert = B[OL_VERT].as<uint8_t>();
  int32_t* zv = B[OL_ZV].as<int32_t>();
  int32_t* dest = B[OL_DEST].as<int32_t>();
  int32_t* slot = B[OL_SLOT].as<int32_t>();
  int32_t* mn[2] = {B[OL_MN0].as<int32_t>(), B[OL_MN1].as<int32_t>()};
  int32_t* nx[2] = {B[OL_NX0].as<int32_t>(), B[OL_NX1].as<int32_t>()};
  int32_t* val[2] = {B[OL_VAL0].as<int32_t>(), B[OL_VAL1].as<int32_t>()};
  const int nb = nblk(n, 256);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  outline_compact_kernel<<<grid_of(npix), 256, 0, st>>>(flags, base, npix, n, hnum, d_err);
  outline_succ_kernel<<<nb, 256, 0, st>>>(Image{d_label, w, h}, d_top, flags, base, hnum, n, succ, vert, zv, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  // ---- leaders: R rounds, the first from the successor table itself ----
  int cur = 0;
  outline_min_kernel<<<nb, 256, 0, st>>>(nullptr, succ, n, mn[0], nx[0], d_err);
  for (int r = 1; r < R; r++, cur ^= 1)
    outline_min_kernel<<<nb, 256, 0, st>>>(mn[cur], nx[cur], n, mn[cur ^ 1], nx[cur ^ 1], d_err);
  const int32_t* leader = mn[cur];
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  // ---- rank: the cut, R Wyllie rounds ----
  int cw = 0;  // (the two successor buffers of the leaders are free again)
  outline_cut_kernel<<<nb, 256, 0, st>>>(succ, leader, vert, n, nx[0], val[0]);
  for (int r = 0; r < R; r++, cw ^= 1)
    outline_jump_kernel<<<nb, 256, 0, st>>>(nx[cw], val[cw], n, nx[cw ^ 1], val[cw ^ 1], d_err);
  const int32_t* suffix = val[cw];
  BS_HIP(ctx, hipEventRecord(ev.e[5], st));
  // ---- rings: a slot per leader ----
  hipcub::TransformInputIterator<int32_t, LeadFlag, hipcub::CountingInputIterator<int32_t>> leads(idx, LeadFlag{leader});
  BS_HIP(ctx, cub_run(B[OL_TMP], [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, leads, slot, n, st); }));
  BS_HIP(ctx, hipEventRecord(ev.e[6], st));
  int h_err = 0;
  int32_t last_slot = 0, last_leader = -1;
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_slot, slot + n - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&last_leader, leader + n - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // round trip 2: n_rings
  BS_HIP(ctx, hipGetLastError());
  if (h_err || R < 2)
    return internal(ctx, h_err);
  const int64_t n_rings = (int64_t)last_slot + (last_leader == n - 1);
  if (n_rings < 1 || 4 * n_rings > n_half)
    return internal(ctx, 0x100);
  const int32_t nr = (int32_t)n_rings;
  const bool ok[] = {alloc(&res.ring_label, nr),  alloc(&res.ring_start, nr),    alloc(&res.ring_length, nr), alloc(&res.ring_vertices, nr),
                     alloc(&res.ring_area2, nr),  alloc(&res.ring_bbox, 4 * (size_t)nr), alloc(&res.ring_offset, (size_t)nr + 1)};
  if (!std::all_of(std::begin(ok), std::end(ok), [](bool b) { return b; }))
    return fail(ctx, BS_ERR_NOMEM, "facet outlines: host allocation");
  BS_HIP(ctx, B[OL_KEYS].reserve(8 * (size_t)nr));
  BS_HIP(ctx, B[OL_KEYS2].reserve(8 * (size_t)nr));
  BS_HIP(ctx, B[OL_VALS].reserve(4 * (size_t)nr));
  BS_HIP(ctx, B[OL_VALS2].reserve(4 * (size_t)nr));
  BS_HIP(ctx, B[OL_RSLOT].reserve(SLOT_FIG_BYTES * (size_t)nr));
  BS_HIP(ctx, B[OL_RING].reserve(RING_OUT_BYTES * (size_t)nr + 4));
  BS_HIP(ctx, B[OL_LRO].reserve(4 * ((size_t)n_labels + 1)));
  unsigned long long* keys = B[OL_KEYS].as<unsigned long long>();
  unsigned long long* skeys = B[OL_KEYS2].as<unsigned long long>();
  int32_t* vals = B[OL_VALS].as<int32_t>();
  int32_t* svals = B[OL_VALS2].as<int32_t>();
  int32_t* lro = B[OL_LRO].as<int32_t>();
  const SlotFig F = slot_fig_at(B[OL_RSLOT].p, (size_t)nr);
  const RingOut RO = ring_out_at(B[OL_RING].p, (size_t)nr);
  const int end_bit = 32 + bits_of(n_labels);
  hipcub::TransformInputIterator<int32_t, VertexCount, hipcub::CountingInputIterator<int32_t>> counts(idx,
                                                                                                      VertexCount{RO.vertices, nr});
  auto sort = [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys, skeys, vals, svals, nr, 0, end_bit, st);
  };
  auto offsets = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, counts, RO.offset, nr + 1, st); };
  BS_HIP(ctx, cub_room(B[OL_TMP], sort, offsets));
  BS_HIP(ctx, hipEventRecord(ev.e[7], st));
  outline_slot_init_kernel<<<nblk(nr, 256), 256, 0, st>>>(F, nr);
  outline_figures_kernel<<<grid_of(n), 256, 0, st>>>(hnum, leader, slot, suffix, d_label, w, n, nr, keys, vals, F, d_err);
  BS_HIP(ctx, cub_run_sized(B[OL_TMP], sort));
  outline_gather_kernel<<<nblk(nr, 256), 256, 0, st>>>(skeys, svals, nr, F, RO, d_err);
  BS_HIP(ctx, cub_run_sized(B[OL_TMP], offsets));
  outline_label_offset_kernel<<<nblk((int64_t)n_labels + 1, 256), 256, 0, st>>>(RO.label, nr, n_labels, bits_of(nr) + 1, lro);
  outline_place_kernel<<<nb, 256, 0, st>>>(vert, leader, slot, suffix, nx[cw], n, nr, RO, dest, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[8], st));
  std::vector<int32_t> i32(4 * (size_t)nr + 1 + (size_t)n_labels + 1);
  int32_t* h_label = i32.data();
  int32_t* h_start = h_label + nr;
  int32_t* h_vertices = h_start + nr;
  int32_t* h_offset = h_vertices + nr;  // [nr + 1]
  int32_t* h_lro = h_offset + nr + 1;   // [n_labels + 1]
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_label, RO.label, 4 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_start, RO.start, 4 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_vertices, RO.vertices, 4 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_offset, RO.offset, 4 * ((size_t)nr + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_lro, lro, 4 * ((size_t)n_labels + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.ring_length, RO.length, 8 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.ring_area2, RO.area2, 8 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.ring_bbox, RO.bbox, 16 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // round trip 3: n_vertices
  BS_HIP(ctx, hipGetLastError());
  if (h_err)
    return internal(ctx, h_err);
  int64_t sum_len = 0;
  for (int32_t r = 0; r < nr; r++) {
    res.ring_label[r] = h_label[r];
    res.ring_start[r] = h_start[r];
    res.ring_vertices[r] = h_vertices[r];
    res.ring_offset[r] = h_offset[r];
    sum_len += res.ring_length[r];
  }
  res.ring_offset[nr] = h_offset[nr];
  for (int64_t l = 0; l <= n_labels; l++)
    res.label_ring_offset[l] = h_lro[l];
  if (sum_len != n_half || h_offset[nr] < 4 || h_offset[nr] > n)
    return internal(ctx, 0x200);
  res.n_half = n_half;
  res.n_rings = n_rings;
  res.n_vertices = h_offset[nr];
  res.ms_halfedges += ev.ms(2, 3);
  res.ms_leaders = ev.ms(3, 4);
  res.ms_rank = ev.ms(4, 5);
  res.ms_rings = ev.ms(5, 6) + ev.ms(7, 8);
  ctx->ol_nhalf = n_half;
  ctx->ol_nv = res.n_vertices;
  ctx->ol_w = w;
  ctx->ol_nr = nr;
  ctx->ol_leader = leader;
  ctx->ol_has_z = d_top != nullptr;
  ctx->ol_valid = true;
  *out = res;
  guard.keep = true;
  return BS_OK;
}

extern "C" int bs_facet_outlines_emit_dev(bs_ctx* ctx, int32_t* d_xy, int32_t* d_z)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!ctx->ol_valid)
    return fail(ctx, BS_ERR_INVALID, "facet outlines: emit without a successful count on this context");
  if ((ctx->ol_nv > 0 && !d_xy) || (ctx->ol_nv > 0 && ctx->ol_has_z && !d_z) || (!ctx->ol_has_z && d_z))
    return fail(ctx, BS_ERR_INVALID, "facet outlines: emit needs d_xy, and d_z exactly when the count had a top image");
  ctx->ol_ms_emit = 0;
  if (ctx->ol_nv == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->ol;
  Events<2> ev;
  BS_HIP(ctx, hipEventCreate(&ev.e[0]));
  BS_HIP(ctx, hipEventCreate(&ev.e[1]));
  const int32_t n = (int32_t)ctx->ol_nhalf;
  int* d_err = B[OL_MISC].as<int>() + 1;
  BS_HIP(ctx, hipMemsetAsync(d_err, 0, 4, st));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  outline_emit_kernel<<<nblk(n, 256), 256, 0, st>>>(B[OL_HNUM].as<int32_t>(), B[OL_DEST].as<int32_t>(), B[OL_ZV].as<int32_t>(),
                                                    ctx->ol_w, n, (int32_t)ctx->ol_nv, reinterpret_cast<int2*>(d_xy), d_z, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  int h_err = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_err)
    return internal(ctx, h_err);
  ctx->ol_ms_emit = ev.ms(0, 1);
  return BS_OK;
}

extern "C" int bs_facet_outlines(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height,
                                 int32_t n_labels, struct bs_outlines* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->ol_valid = false;
  if (!label || !out || bad_image(width, height) || n_labels < 0)
    return fail(ctx, BS_ERR_INVALID, OUTLINES_INVALID);
  const size_t npix = (size_t)width * height;
  DevBuf* B = ctx->ol;
  Staging S(ctx);
  const int32_t* d_label = S.upload(B[OL_IN_LABEL], label, npix);
  const int32_t* d_top = S.upload(B[OL_IN_TOP], top, 4 * npix);
  if (!S.ok())
    return S.status();
  struct bs_outlines res;
  int rc = bs_facet_outlines_count_dev(ctx, d_label, d_top, width, height, n_labels, &res);
  if (rc != BS_OK)
    return rc;
  Guard guard{&res};
  const size_t nv = (size_t)res.n_vertices;
  if (!alloc(&res.xy, 2 * nv) || (top && !alloc(&res.z, nv)))
    return fail(ctx, BS_ERR_NOMEM, "facet outlines: host allocation");
  if (nv > 0) {
    int32_t* d_xy = S.room<int32_t>(B[OL_OUT_XY], 2 * nv);
    int32_t* d_z = S.room<int32_t>(B[OL_OUT_Z], nv, top != nullptr);
    if (!S.ok())
      return S.status();
    rc = bs_facet_outlines_emit_dev(ctx, d_xy, d_z);
    if (rc != BS_OK)
      return rc;
    S.download(res.xy, d_xy, 2 * nv);
    S.download(res.z, d_z, nv);
    rc = S.finish();
    if (rc != BS_OK)
      return rc;
    res.ms_emit = ctx->ol_ms_emit;
  }
  *out = res;
  guard.keep = true;
  return BS_OK;
}

// The format is written down in include/bs_api.h.
extern "C" int bs_outlines_write_obj(const struct bs_outlines* o, int32_t bin, const int32_t* origin, const char* path)
{
  if (!o || !path || bin < 1 || o->n_rings < 0 || o->n_vertices < 0 || o->n_labels < 0)
    return BS_ERR_INVALID;
  if (!o->ring_offset || !o->label_ring_offset || (o->n_rings > 0 && (!o->ring_label || !o->ring_area2)) ||
      (o->n_vertices > 0 && !o->xy))
    return BS_ERR_INVALID;
  if (o->ring_offset[0] != 0 || o->ring_offset[o->n_rings] != o->n_vertices)
    return BS_ERR_INVALID;
  for (int64_t r = 0; r < o->n_rings; r++) {
    const int32_t l = o->ring_label[r];
    if (o->ring_offset[r + 1] < o->ring_offset[r] || l < 0 || l >= o->n_labels || o->label_ring_offset[l] > r)
      return BS_ERR_INVALID;
  }
  FILE* fo = fopen(path, "w");
  if (!fo)
    return BS_ERR_INVALID;
  const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  fprintf(fo, "# facet outlines: %d labels, %lld rings, %lld vertices\n", o->n_labels, (long long)o->n_rings,
          (long long)o->n_vertices);
  for (int64_t r = 0; r < o->n_rings; r++) {
    const int32_t l = o->ring_label[r];
    fprintf(fo, "g label_%d_ring_%lld_%s\n", l, (long long)(r - o->label_ring_offset[l]), o->ring_area2[r] > 0 ? "outer" : "hole");
    const int64_t a = o->ring_offset[r], b = o->ring_offset[r + 1];
    for (int64_t v = a; v < b; v++)
      fprintf(fo, "v %lld %lld %lld\n", (long long)((int64_t)o->xy[2 * v] * bin + org[0]),
              (long long)((int64_t)o->xy[2 * v + 1] * bin + org[1]), (long long)((o->z ? (int64_t)o->z[v] : 0) + org[2]));
    fputs("l", fo);
    for (int64_t v = a; v < b; v++)
      fprintf(fo, " %lld", (long long)(v + 1));
    fprintf(fo, " %lld\n", (long long)(a + 1));
  }
  const bool ok = !ferror(fo);
  return (fclose(fo) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}
