// bs_trispan.h -- the scan conversion of the outline triangles that the model raster (bs_modelraster.hip) and the point
// residuals (bs_pointresid.hip) share: slots -> pixel rows -> spans -> items, every item found again by bisection
// (DESIGN.md "Model raster" and "Point residuals", each under "The shared triangle scan").  What a span IS differs between the two and stays in their
// files: the pixels whose centres a triangle covers there, the pixels a triangle touches here.  The bits that a failed
// check sets in a file's error word are that file's and come in as arguments.  Everything is internal to a translation
// unit.
#pragma once

#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstdio>

#include "bs_common.h"
#include "bs_host.h"

namespace bs {
namespace {

struct TriCountDev {  // what bs_outline_triangles_count_dev left on the device
  const int2* xy;
  const int32_t* z;
  const int32_t* tri;
  const long long* toff;  // tri_offset [nl + 1]
  int32_t nsv, nl, w, h;
  long long ntri;
};

inline int fail_as(bs_ctx* ctx, int status, const char* who, const char* what)
{
  char msg[128];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return fail(ctx, status, msg);
}

// A from the last triangle count on ctx; BS_ERR_INVALID, worded for `who`, where there is none or it had no top image
inline int tri_count_dev(bs_ctx* ctx, const char* who, TriCountDev& A)
{
  if (!ctx->tr_valid || !ctx->uc_valid)
    return fail_as(ctx, BS_ERR_INVALID, who, "no successful triangle count on this context");
  if (!ctx->uc_has_z)
    return fail_as(ctx, BS_ERR_INVALID, who, "the triangle count had no top image");
  A = TriCountDev{ctx->uc_xy, ctx->uc_z, ctx->tr_tri, ctx->tr_toff, (int32_t)ctx->uc_nsv, ctx->tr_nl, ctx->tr_w, ctx->tr_h,
                  ctx->tr_tri && ctx->tr_toff ? ctx->tr_ntri : 0};
  return BS_OK;
}

// a slot is numbered in 31 bits; the caller's status where there are more (the two stages differ in it), at the place in
// the order of its own checks where the caller asks
inline int check_slots(bs_ctx* ctx, const char* who, const TriCountDev& A, int status)
{
  return A.ntri >= INT32_MAX ? fail_as(ctx, status, who, "2^31 triangle slots or more") : BS_OK;
}

// the three clean vertices of slot t, checked; false for a slot of -1 (a failed label's), and with e_tri in err for any
// other index outside the vertices
__device__ inline bool tri_of(const TriCountDev& A, long long t, int32_t& a, int32_t& b, int32_t& c, int* err, int e_tri)
{
  a = A.tri[3 * t];
  b = A.tri[3 * t + 1];
  c = A.tri[3 * t + 2];
  if (a == -1 && b == -1 && c == -1)
    return false;
  if ((uint32_t)a >= (uint32_t)A.nsv || (uint32_t)b >= (uint32_t)A.nsv || (uint32_t)c >= (uint32_t)A.nsv) {
    atomicOr(err, e_tri);
    return false;
  }
  return true;
}

constexpr int32_t Z_LIMIT = 1 << 24;  // every height of the chain lies strictly inside -Z_LIMIT .. Z_LIMIT

// the range check of the three sz of a slot
__device__ inline bool sz_in_range(int32_t za, int32_t zb, int32_t zc)
{
  return !(za >= Z_LIMIT || za <= -Z_LIMIT || zb >= Z_LIMIT || zb <= -Z_LIMIT || zc >= Z_LIMIT || zc <= -Z_LIMIT);
}

// the pixel rows y0 .. y1 - 1 of an image of h rows between the lowest and the highest corner of a triangle
__device__ inline void rows_of(int32_t h, int2 a, int2 b, int2 c, int32_t& y0, int32_t& y1)
{
  y0 = max(min(a.y, min(b.y, c.y)), 0);
  y1 = min(max(a.y, max(b.y, c.y)), h);
}

// the last k in 0 .. n - 1 with scan[k] <= i, searched between lo and hi (scan is an exclusive sum: scan[0] = 0)
__device__ inline long long last_le(const long long* __restrict__ scan, long long lo, long long hi, long long i)
{
  while (lo < hi) {
    const long long mid = (lo + hi + 1) >> 1;
    if (scan[mid] <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

// the label of triangle slot q: the last l with toff[l] <= q
__device__ inline int32_t label_of_slot(const long long* __restrict__ toff, int32_t nl, long long q)
{
  return (int32_t)last_le(toff, 0, nl - 1, q);
}

struct RowCount {  // 0 for the entry behind the last
  const int32_t* cnt;
  long long n;
  __host__ __device__ long long operator()(long long i) const { return i < n ? cnt[i] : 0; }
};
struct SpanCount {
  const int4* rows;
  long long n;
  __host__ __device__ long long operator()(long long i) const { return i < n ? rows[i].w : 0; }
};
using Idx64 = hipcub::CountingInputIterator<long long>;

// scan[0 .. n] = the exclusive sum of count(0 .. n), count = RowCount or SpanCount over n entries; tmp grows as needed;
// the copy of scan[n] to *total is enqueued behind it, and the caller synchronises where it reads
template <class Count>
hipError_t scan_counts(DevBuf& tmp, const Count& count, long long n, long long* scan, long long* total, hipStream_t st)
{
  using It = hipcub::TransformInputIterator<long long, Count, Idx64>;  // (the type the two files have always scanned over)
  hipError_t e = cub_run(tmp, [&](void* t, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(t, bytes, It(Idx64(0), count), scan, (int)(n + 1), st);
  });
  if (e == hipSuccess)
    e = hipMemcpyAsync(total, scan + n, 8, hipMemcpyDeviceToHost, st);
  return e;
}

// the head of a spans kernel: row item r is row y of slot t with the corners pa, pb, pc.  False with e_row in err where the
// slot has no such row (a slot of -1 has none at all), and then only t, and y where the slot has corners, are set
__device__ inline bool row_of(const TriCountDev& A, const long long* __restrict__ rowscan, long long r, long long& t, int2& pa,
                              int2& pb, int2& pc, int32_t& y, int* err, int e_tri, int e_row)
{
  t = last_le(rowscan, 0, A.ntri - 1, r);
  int32_t a, b, c;
  if (tri_of(A, t, a, b, c, err, e_tri)) {
    pa = A.xy[a], pb = A.xy[b], pc = A.xy[c];
    int32_t y0, y1;
    rows_of(A.h, pa, pb, pc, y0, y1);
    y = y0 + (int32_t)(r - rowscan[t]);
    if (y >= y0 && y < y1)
      return true;
  }
  atomicOr(err, e_row);
  return false;
}

// the tail of a spans kernel: the columns first .. last of a row, clipped to an image of w columns, as (x0, len); both stay
// as they are where nothing is left
__device__ inline void clip_span(int32_t w, long long first, long long last, int32_t& x0, int32_t& len)
{
  const long long f = max(first, 0ll), l = min(last, (long long)w - 1);
  if (f <= l) {
    x0 = (int32_t)f;
    len = (int32_t)(l - f + 1);
  }
}

// item i of a chunk whose first and last item lie in the row items s_row[0] and s_row[1] (bisected by the workgroup): a
// thread bisects between the two.  The slot and the pixel of the item, checked; false with e_item in err
__device__ inline bool item_of(const TriCountDev& A, const long long* __restrict__ spanscan, const int4* __restrict__ rows,
                               const long long* s_row, long long i, int32_t& slot, long long& x, int32_t& y, int* err, int e_item)
{
  const long long r = last_le(spanscan, s_row[0], s_row[1], i);
  const int4 rec = rows[r];
  const long long off = i - spanscan[r];
  slot = rec.x;
  x = rec.z + off;
  y = rec.y;
  if (off < 0 || off >= rec.w || (uint32_t)slot >= (uint64_t)A.ntri || (uint32_t)y >= (uint32_t)A.h || x < 0 || x >= A.w) {
    atomicOr(err, e_item);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace bs
