// bs_modelraster.hip -- model raster: the outline triangles back on the pixel lattice, and the model's error against the label
// image and top (DESIGN.md "Model raster"; the definition is written down in include/bs_api.h under "model raster").
//   input     bs_outline_triangles_count_dev on the context: the clean vertices with Z (bs_ctx::uc_xy, uc_z), the triangles
//             (tr_tri) and tri_offset (tr_toff) stay on the device; nothing of it is written
//   rows      per slot the pixel rows its box crosses (0 for a slot of -1); one exclusive sum: the row items
//   spans     per row item the pixels whose centres lie between the two edge crossings of the row's centre line, by exact
//             integer ceiling and floor (often none for a sliver); one exclusive sum: the pixel items
//   pixels    one thread per pixel item: a workgroup bisects the span offsets for the first and the last item of its chunk,
//             a thread bisects between the two; the three weights with the tie rule; where covered one atomicMin on win and
//             one atomicAdd on cover, both without return
//   figures   one pass over the pixels: the winner's weights again, M, mz2, e2; the per-label figures reduced as
//             bs_polysolid.hip reduces its own: a wave inside one (L, M) in registers, labels below FIG_CAP through LDS
//             tables, the rest by global atomics
// No work item's time grows with a triangle's box or area.  Every index read from memory is checked before it is used as an
// address; a violation sets err and the call returns BS_ERR_INTERNAL.  The three images are built in scratch and copied to
// the caller's only after the last check, so that an error leaves them untouched.
// The walk from slots to rows to spans to items is bs_trispan.h's, shared with bs_pointresid.hip; what a span is (crossing,
// below) is this file's.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_chain.h"
#include "bs_common.h"
#include "bs_host.h"
#include "bs_trispan.h"

namespace bs {
namespace {

// scratch of bs_ctx::mr
enum { MR_MISC, MR_TMP, MR_ROWCNT, MR_ROWSCAN, MR_ROWS, MR_SPANSCAN, MR_WIN, MR_COVER, MR_MZ2, MR_FIG, MR_IN_LABEL, MR_IN_TOP,
       MR_OUT, MR_COUNT };
static_assert(MR_COUNT <= (int)(sizeof(bs_ctx::mr) / sizeof(DevBuf)), "bs_ctx::mr is too short");

constexpr int FIG_CAP = BS_MRASTER_FIG_CAP;  // labels 0 .. FIG_CAP - 1: figures reduced in LDS (24 KiB in mr_figures_kernel)
constexpr int CHUNK = BS_MRASTER_CHUNK;      // pixel items of one workgroup
constexpr int CHUNK_GRID = 1 << 20;          // workgroups of the pixel pass; beyond, a workgroup takes several chunks
constexpr int FIG_GRID = BS_MRASTER_FIG_GRID;  // workgroups of the figures pass (its LDS tables let six of them share a CU)
constexpr unsigned NO_SLOT = ~0u;
enum { W_ERR, W_RANGE, W_WORDS = 4 };                                                  // the int words of MR_MISC
enum { C_UNCOVERED, C_SPILL, C_MOVED, C_MULTI, C_COVER, C_EMPTY, C_MAXSPAN, C_COUNT };  // its 64-bit counters, behind the words
enum { E_TRI = 1, E_ROW = 2, E_ITEM = 4, E_WIN = 8 };                                   // the bits of W_ERR
enum { F_PIXELS, F_MODEL, F_KEPT, F_MULTI, F_ERRP, F_SABS, F_MABS, F_SQLO, F_SQHI, F_COUNT };  // the arrays of MR_FIG

__device__ inline bool owns(long long w, bool up) { return w > 0 || (w == 0 && up); }

// the weights of the centre of pixel (x, y) in the triangle a, b, c (lattice corners), in doubled units; true iff covered
__device__ inline bool weights_of(int2 a, int2 b, int2 c, int32_t x, int32_t y, long long& wa, long long& wb, long long& wc)
{
  const long long px = 2ll * x + 1, py = 2ll * y + 1;
  const long long ax = 2ll * a.x - px, ay = 2ll * a.y - py, bx = 2ll * b.x - px, by = 2ll * b.y - py, cx = 2ll * c.x - px,
                  cy = 2ll * c.y - py;
  wa = bx * cy - by * cx;  // orient(P, B, C), edge B -> C
  wb = cx * ay - cy * ax;  // orient(P, C, A), edge C -> A
  wc = ax * by - ay * bx;  // orient(P, A, B), edge A -> B
  return owns(wa, c.y > b.y) && owns(wb, a.y > c.y) && owns(wc, b.y > a.y);
}

// ---- 1. rows --------------------------------------------------------------------------------------------------------------
// (the rows of a slot: those whose centre line crosses the box of the triangle)
__global__ __launch_bounds__(256) void mr_rows_kernel(TriCountDev A, int32_t* __restrict__ rowcnt, int* __restrict__ words)
{
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < A.ntri; t += (long long)gridDim.x * blockDim.x) {
    int32_t a, b, c, cnt = 0;
    if (tri_of(A, t, a, b, c, words + W_ERR, E_TRI)) {
      if (!sz_in_range(A.z[a], A.z[b], A.z[c]))
        atomicOr(words + W_RANGE, 1);
      int32_t y0, y1;
      rows_of(A.h, A.xy[a], A.xy[b], A.xy[c], y0, y1);
      cnt = max(y1 - y0, 0);
    }
    rowcnt[t] = cnt;
  }
}

// ---- 2. spans -------------------------------------------------------------------------------------------------------------
// the crossing of the edge u -> v (doubled units) with the line Y = yc, which is odd and so passes no vertex, at
// X = ux + num / den: the first pixel whose centre 2 x + 1 is not left of it, and the last whose centre is not right of it, by
// exact integer ceiling and floor of ((ux - 1) den + num) / (2 den)
__device__ inline void crossing(long long ux, long long uy, long long vx, long long vy, long long yc, long long& first, long long& last)
{
  if ((uy < yc) == (vy < yc))
    return;
  long long den = vy - uy, num = (vx - ux) * (yc - uy);
  if (den < 0) {
    den = -den;
    num = -num;
  }
  const long long n = (ux - 1) * den + num, d = 2 * den;
  long long q = n / d;
  const long long rem = n - q * d;
  if (rem < 0)
    q--;
  first = min(first, q + (rem != 0));
  last = max(last, q);
}

__global__ __launch_bounds__(256) void mr_spans_kernel(TriCountDev A, const long long* __restrict__ rowscan, long long n_rows,
                                                       int4* __restrict__ rows, int* __restrict__ words,
                                                       unsigned long long* __restrict__ counters)
{
  unsigned empties = 0;
  int32_t longest = 0;
  for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n_rows; r += (long long)gridDim.x * blockDim.x) {
    long long t;
    int2 pa, pb, pc;
    int32_t x0 = 0, len = 0, y = 0;
    if (row_of(A, rowscan, r, t, pa, pb, pc, y, words + W_ERR, E_TRI, E_ROW)) {
      const long long yc = 2ll * y + 1;
      long long xlo = LLONG_MAX, xhi = LLONG_MIN;
      crossing(2ll * pb.x, 2ll * pb.y, 2ll * pc.x, 2ll * pc.y, yc, xlo, xhi);
      crossing(2ll * pc.x, 2ll * pc.y, 2ll * pa.x, 2ll * pa.y, yc, xlo, xhi);
      crossing(2ll * pa.x, 2ll * pa.y, 2ll * pb.x, 2ll * pb.y, yc, xlo, xhi);
      if (xlo != LLONG_MAX)  // the pixels xlo .. xhi have their centres between the two crossings
        clip_span(A.w, xlo, xhi, x0, len);
    }
    rows[r] = make_int4((int32_t)t, y, x0, len);
    empties += len == 0;
    longest = max(longest, len);
  }
  for (int o = 32; o > 0; o >>= 1) {
    empties += __shfl_xor(empties, o);
    longest = max(longest, __shfl_xor(longest, o));
  }
  if ((threadIdx.x & 63) == 0) {
    if (empties)
      atomicAdd(counters + C_EMPTY, (unsigned long long)empties);
    if (longest)
      atomicMax(counters + C_MAXSPAN, (unsigned long long)longest);
  }
}

// ---- 3. pixel items -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CHUNK) void mr_pixels_kernel(TriCountDev A, const long long* __restrict__ spanscan,
                                                          const int4* __restrict__ rows, long long n_rows, long long n_items,
                                                          unsigned* __restrict__ win, unsigned* __restrict__ cover,
                                                          int* __restrict__ err)
{
  __shared__ long long s_row[2];  // the rows of the first and of the last item of the chunk
  const long long n_chunks = (n_items + CHUNK - 1) / CHUNK;
  for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const long long base = chunk * CHUNK, last = min(base + CHUNK, n_items) - 1;
    if (threadIdx.x < 2)
      s_row[threadIdx.x] = last_le(spanscan, 0, n_rows - 1, threadIdx.x == 0 ? base : last);
    __syncthreads();
    const long long i = base + threadIdx.x;
    if (i <= last) {
      int32_t slot, y, a, b, c;
      long long x;
      if (item_of(A, spanscan, rows, s_row, i, slot, x, y, err, E_ITEM) && tri_of(A, slot, a, b, c, err, E_TRI)) {
        long long wa, wb, wc;
        if (weights_of(A.xy[a], A.xy[b], A.xy[c], (int32_t)x, y, wa, wb, wc)) {
          const long long p = (long long)y * A.w + x;
          atomicMin(win + p, (unsigned)slot);
          atomicAdd(cover + p, 1u);
        }
      }
    }
    __syncthreads();
  }
}

// ---- 4. figures -----------------------------------------------------------------------------------------------------------
struct Fig {  // per label, device
  unsigned long long* f[F_COUNT];
};

struct Tables {  // the figures of the labels below FIG_CAP, in LDS
  unsigned cnt[5][FIG_CAP];  // F_PIXELS .. F_ERRP
  unsigned mabs[FIG_CAP];
  unsigned long long sabs[FIG_CAP], sqlo[FIG_CAP], sqhi[FIG_CAP];
};

__device__ inline void add_count(Tables& T, const Fig& f, int which, int32_t l, unsigned v)
{
  if (!v)
    return;
  if (l < FIG_CAP)
    atomicAdd(&T.cnt[which][l], v);
  else
    atomicAdd(f.f[which] + l, (unsigned long long)v);
}

__device__ inline void add_error(Tables& T, const Fig& f, int32_t l, unsigned long long sabs, unsigned mabs, unsigned long long sqlo,
                                 unsigned long long sqhi)
{
  if (l < FIG_CAP) {
    if (sabs)
      atomicAdd(&T.sabs[l], sabs);
    if (mabs)
      atomicMax(&T.mabs[l], mabs);
    if (sqlo)
      atomicAdd(&T.sqlo[l], sqlo);
    if (sqhi)
      atomicAdd(&T.sqhi[l], sqhi);
  } else {
    if (sabs)
      atomicAdd(f.f[F_SABS] + l, sabs);
    if (mabs)
      atomicMax(f.f[F_MABS] + l, (unsigned long long)mabs);
    if (sqlo)
      atomicAdd(f.f[F_SQLO] + l, sqlo);
    if (sqhi)
      atomicAdd(f.f[F_SQHI] + l, sqhi);
  }
}

// win holds the winning slot of every pixel (NO_SLOT: none) and leaves as M
__global__ __launch_bounds__(256) void mr_figures_kernel(TriCountDev A, const int32_t* __restrict__ label,
                                                         const int32_t* __restrict__ top, long long npix, int32_t* win,
                                                         const unsigned* __restrict__ cover, int32_t* __restrict__ mz2, Fig f,
                                                         int* __restrict__ words, unsigned long long* __restrict__ counters)
{
  __shared__ Tables T;
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    for (int j = 0; j < 5; j++)
      T.cnt[j][k] = 0;
    T.mabs[k] = 0;
    T.sabs[k] = T.sqlo[k] = T.sqhi[k] = 0;
  }
  __syncthreads();
  unsigned n_unc = 0, n_spill = 0, n_moved = 0, n_multi = 0;
  unsigned long long n_cover = 0;
  const long long n64 = (npix + 63) & ~63ll;  // whole waves stay together
  for (long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x; p < n64; p += (long long)gridDim.x * blockDim.x) {
    int32_t L = -1, M = -1;
    unsigned cov = 0, mabs = 0, has_e = 0;
    unsigned long long sqlo = 0, sqhi = 0;
    if (p < npix) {
      L = label[p];
      if ((uint32_t)L >= (uint32_t)A.nl)
        L = -1;
      cov = cover[p];
      const unsigned t = (unsigned)win[p];
      int32_t h2 = INT32_MIN, a, b, c;
      if (t != NO_SLOT) {
        if (t >= (unsigned long long)A.ntri || !tri_of(A, t, a, b, c, words + W_ERR, E_TRI)) {
          atomicOr(words + W_ERR, E_WIN);
        } else {
          const int32_t y = (int32_t)((uint32_t)p / (uint32_t)A.w), x = (int32_t)((uint32_t)p - (uint32_t)y * (uint32_t)A.w);  // (p < 2^29)
          long long wa, wb, wc;
          weights_of(A.xy[a], A.xy[b], A.xy[c], x, y, wa, wb, wc);
          const long long D = wa + wb + wc, N = wa * A.z[a] + wb * A.z[b] + wc * A.z[c];
          if (D <= 0) {
            atomicOr(words + W_ERR, E_WIN);
          } else {
            const long long num = 4 * N + D, den = 2 * D;
            long long q = num / den;
            if (num - q * den < 0)
              q--;
            h2 = (int32_t)q;
            M = label_of_slot(A.toff, A.nl, t);
          }
        }
      }
      win[p] = M;
      mz2[p] = h2;
      if (L >= 0 && M >= 0) {
        const long long s = (long long)top[4 * p] + top[4 * p + 3];  // t00 + t11
        if (s >= 2ll * Z_LIMIT || s <= -2ll * Z_LIMIT) {
          atomicOr(words + W_RANGE, 2);
        } else {
          const long long e = (long long)h2 - s;
          const unsigned long long ae = (unsigned long long)(e < 0 ? -e : e), sq = ae * ae;
          has_e = 1;
          mabs = (unsigned)ae;
          sqlo = sq & 0xFFFFFFFFull;
          sqhi = sq >> 32;
        }
      }
      n_unc += L >= 0 && M < 0;
      n_spill += L < 0 && M >= 0;
      n_moved += L >= 0 && M >= 0 && L != M;
      n_multi += cov > 1;
      n_cover += cov;
    }
    const int32_t L0 = __shfl(L, 0), M0 = __shfl(M, 0);
    if (__all(L == L0 && M == M0)) {  // the whole wave inside one label of the image and one of the model: registers
      if (L0 < 0 && M0 < 0)
        continue;
      unsigned multi = cov > 1, errp = has_e, mx = mabs;
      unsigned long long sabs = mabs;
      for (int o = 32; o > 0; o >>= 1) {
        multi += __shfl_xor(multi, o);
        errp += __shfl_xor(errp, o);
        mx = max(mx, __shfl_xor(mx, o));
        sabs += __shfl_xor(sabs, o);
        sqlo += __shfl_xor(sqlo, o);
        sqhi += __shfl_xor(sqhi, o);
      }
      if ((threadIdx.x & 63) == 0) {
        if (L0 >= 0)
          add_count(T, f, F_PIXELS, L0, 64);
        if (M0 >= 0) {
          add_count(T, f, F_MODEL, M0, 64);
          add_count(T, f, F_KEPT, M0, L0 == M0 ? 64 : 0);
          add_count(T, f, F_MULTI, M0, multi);
          add_count(T, f, F_ERRP, M0, errp);
          add_error(T, f, M0, sabs, mx, sqlo, sqhi);
        }
      }
    } else {
      if (L >= 0)
        add_count(T, f, F_PIXELS, L, 1);
      if (M >= 0) {
        add_count(T, f, F_MODEL, M, 1);
        add_count(T, f, F_KEPT, M, L == M);
        add_count(T, f, F_MULTI, M, cov > 1);
        add_count(T, f, F_ERRP, M, has_e);
        if (has_e)
          add_error(T, f, M, mabs, mabs, sqlo, sqhi);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_unc += __shfl_xor(n_unc, o);
    n_spill += __shfl_xor(n_spill, o);
    n_moved += __shfl_xor(n_moved, o);
    n_multi += __shfl_xor(n_multi, o);
    n_cover += __shfl_xor(n_cover, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_unc)
      atomicAdd(counters + C_UNCOVERED, (unsigned long long)n_unc);
    if (n_spill)
      atomicAdd(counters + C_SPILL, (unsigned long long)n_spill);
    if (n_moved)
      atomicAdd(counters + C_MOVED, (unsigned long long)n_moved);
    if (n_multi)
      atomicAdd(counters + C_MULTI, (unsigned long long)n_multi);
    if (n_cover)
      atomicAdd(counters + C_COVER, n_cover);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < A.nl; k += blockDim.x) {
    for (int j = 0; j < 5; j++)
      if (T.cnt[j][k])
        atomicAdd(f.f[j] + k, (unsigned long long)T.cnt[j][k]);
    if (T.sabs[k])
      atomicAdd(f.f[F_SABS] + k, T.sabs[k]);
    if (T.mabs[k])
      atomicMax(f.f[F_MABS] + k, (unsigned long long)T.mabs[k]);
    if (T.sqlo[k])
      atomicAdd(f.f[F_SQLO] + k, T.sqlo[k]);
    if (T.sqhi[k])
      atomicAdd(f.f[F_SQHI] + k, T.sqhi[k]);
  }
}

int internal(bs_ctx* ctx, int err)
{
  char msg[96];
  snprintf(msg, sizeof msg, "model raster: an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

// the raster of the triangle state on ctx over the device images; res is zeroed; d_model, d_cover, d_mz2 may be NULL
int raster(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height, int32_t* d_model,
           int32_t* d_cover, int32_t* d_mz2, struct bs_model_raster& res)
{
  TriCountDev A;
  int rc = tri_count_dev(ctx, "model raster", A);
  if (rc != BS_OK)
    return rc;
  if (!d_label || !d_top)
    return fail(ctx, BS_ERR_INVALID, "model raster: null pointer");
  if (width != A.w || height != A.h)
    return fail(ctx, BS_ERR_INVALID, "model raster: the image size differs from the triangle count's");
  const int32_t nl = A.nl;
  const long long ntri = A.ntri, npix = (long long)width * height;
  rc = check_slots(ctx, "model raster", A, BS_ERR_INVALID);
  if (rc != BS_OK)
    return rc;
  if (ntri > 0 && (!A.xy || !A.z || nl < 1))
    return internal(ctx, 0x10000);
  res.width = width;
  res.height = height;
  res.n_labels = nl;
  res.fig_cap = FIG_CAP;
  res.chunk = CHUNK;
  res.n_triangles = ctx->tr_ntri;
  const size_t nls = (size_t)std::max(nl, 0);
  int64_t** const arrays[F_COUNT] = {&res.pixels,     &res.model_pixels, &res.kept,  &res.multi, &res.err_pixels,
                                     &res.sum_abs_e2, &res.max_abs_e2,   &res.sq_lo, &res.sq_hi};
  for (auto a : arrays)
    if (!alloc(a, nls))
      return fail(ctx, BS_ERR_NOMEM, "model raster: host allocation");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->mr;
  Events<5> ev;
  for (int i = 0; i < 5; i++)
    BS_HIP(ctx, hipEventCreate(&ev.e[i]));
  const size_t fig_bytes = 8 * (size_t)F_COUNT * std::max<size_t>(nls, 1), misc_bytes = 4 * W_WORDS + 8 * C_COUNT;
  BS_HIP(ctx, B[MR_MISC].reserve(misc_bytes));
  BS_HIP(ctx, B[MR_FIG].reserve(fig_bytes));
  for (int b : {MR_WIN, MR_COVER, MR_MZ2})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[MR_ROWCNT].reserve(4 * (size_t)std::max(ntri, 1ll)));
  BS_HIP(ctx, B[MR_ROWSCAN].reserve(8 * ((size_t)ntri + 1)));
  int* d_words = B[MR_MISC].as<int>();
  unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(d_words + W_WORDS);
  unsigned* win = B[MR_WIN].as<unsigned>();
  unsigned* cover = B[MR_COVER].as<unsigned>();
  int32_t* mz2 = B[MR_MZ2].as<int32_t>();
  int32_t* rowcnt = B[MR_ROWCNT].as<int32_t>();
  long long* rowscan = B[MR_ROWSCAN].as<long long>();
  Fig f;
  for (int j = 0; j < F_COUNT; j++)
    f.f[j] = B[MR_FIG].as<unsigned long long>() + (size_t)j * std::max<size_t>(nls, 1);
  long long n_rows = 0, n_items = 0;
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_words, 0, misc_bytes, st));
  BS_HIP(ctx, hipMemsetAsync(B[MR_FIG].p, 0, fig_bytes, st));
  BS_HIP(ctx, hipMemsetAsync(win, 0xFF, 4 * (size_t)npix, st));
  BS_HIP(ctx, hipMemsetAsync(cover, 0, 4 * (size_t)npix, st));
  if (ntri > 0) {
    // 1. rows
    mr_rows_kernel<<<sweep(ntri), 256, 0, st>>>(A, rowcnt, d_words);
    BS_HIP(ctx, scan_counts(B[MR_TMP], RowCount{rowcnt, ntri}, ntri, rowscan, &n_rows, st));
    BS_HIP(ctx, hipStreamSynchronize(st));  // n_rows
  }
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  if (n_rows >= INT32_MAX)
    return fail(ctx, BS_ERR_INVALID, "model raster: 2^31 row items or more");
  if (n_rows > 0) {
    // 2. spans
    BS_HIP(ctx, B[MR_ROWS].reserve(16 * (size_t)n_rows));
    BS_HIP(ctx, B[MR_SPANSCAN].reserve(8 * ((size_t)n_rows + 1)));
    int4* rows = B[MR_ROWS].as<int4>();
    long long* spanscan = B[MR_SPANSCAN].as<long long>();
    mr_spans_kernel<<<sweep(n_rows), 256, 0, st>>>(A, rowscan, n_rows, rows, d_words, d_counters);
    BS_HIP(ctx, scan_counts(B[MR_TMP], SpanCount{rows, n_rows}, n_rows, spanscan, &n_items, st));
    BS_HIP(ctx, hipStreamSynchronize(st));  // n_items
    BS_HIP(ctx, hipEventRecord(ev.e[2], st));
    // 3. pixel items
    if (n_items > 0) {
      const long long n_chunks = (n_items + CHUNK - 1) / CHUNK;
      mr_pixels_kernel<<<(int)std::min<long long>(n_chunks, CHUNK_GRID), CHUNK, 0, st>>>(A, spanscan, rows, n_rows, n_items, win, cover,
                                                                                         d_words + W_ERR);
    }
  } else {
    BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  }
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  // 4. figures
  mr_figures_kernel<<<(int)std::max<long long>(1, std::min<long long>(nblk(npix, 256), FIG_GRID)), 256, 0, st>>>(A, d_label, d_top, npix, reinterpret_cast<int32_t*>(win),
                                                 cover, mz2, f, d_words, d_counters);
  int h_words[W_WORDS] = {};
  unsigned long long h_counters[C_COUNT] = {};
  std::vector<unsigned long long> h_fig((size_t)F_COUNT * std::max<size_t>(nls, 1));
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_WORDS, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_counters, d_counters, 8 * C_COUNT, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_fig.data(), B[MR_FIG].p, fig_bytes, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  if (h_words[W_ERR])
    return internal(ctx, h_words[W_ERR]);
  if (h_words[W_RANGE] & 1)
    return fail(ctx, BS_ERR_RANGE, "model raster: a vertex of a triangle lies 2^24 or more above or below 0");
  if (h_words[W_RANGE])
    return fail(ctx, BS_ERR_RANGE, "model raster: |t00 + t11| of a pixel is 2^25 or more");
  if (d_model)
    BS_HIP(ctx, hipMemcpyAsync(d_model, win, 4 * (size_t)npix, hipMemcpyDeviceToDevice, st));
  if (d_cover)
    BS_HIP(ctx, hipMemcpyAsync(d_cover, cover, 4 * (size_t)npix, hipMemcpyDeviceToDevice, st));
  if (d_mz2)
    BS_HIP(ctx, hipMemcpyAsync(d_mz2, mz2, 4 * (size_t)npix, hipMemcpyDeviceToDevice, st));
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the copies
  for (int j = 0; j < F_COUNT; j++)
    for (size_t l = 0; l < nls; l++)
      (*arrays[j])[l] = (int64_t)h_fig[(size_t)j * std::max<size_t>(nls, 1) + l];
  for (size_t l = 0; l < nls; l++) {
    res.total_pixels += res.pixels[l];
    res.total_model_pixels += res.model_pixels[l];
    res.total_kept += res.kept[l];
    res.total_err_pixels += res.err_pixels[l];
    res.total_sum_abs_e2 += res.sum_abs_e2[l];
    res.max_abs_e2_all = std::max(res.max_abs_e2_all, res.max_abs_e2[l]);
    res.total_sq_lo += res.sq_lo[l];
    res.total_sq_hi += res.sq_hi[l];
  }
  res.n_uncovered = (int64_t)h_counters[C_UNCOVERED];
  res.n_spill = (int64_t)h_counters[C_SPILL];
  res.n_moved = (int64_t)h_counters[C_MOVED];
  res.n_multi = (int64_t)h_counters[C_MULTI];
  res.sum_cover = (int64_t)h_counters[C_COVER];
  res.n_empty_spans = (int64_t)h_counters[C_EMPTY];
  res.max_span = (int64_t)h_counters[C_MAXSPAN];
  res.n_rows = n_rows;
  res.n_items = n_items;
  res.ms_rows = ev.ms(0, 1);
  res.ms_spans = ev.ms(1, 2);
  res.ms_pixels = ev.ms(2, 3);
  res.ms_figures = ev.ms(3, 4);
  return BS_OK;
}

using ResultGuard = FreeUnlessKept<struct bs_model_raster, bs_model_raster_free>;

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_model_raster_free(struct bs_model_raster* r)
{
  if (!r)
    return;
  free(r->pixels);
  free(r->model_pixels);
  free(r->kept);
  free(r->multi);
  free(r->err_pixels);
  free(r->sum_abs_e2);
  free(r->max_abs_e2);
  free(r->sq_lo);
  free(r->sq_hi);
  memset(r, 0, sizeof *r);
}

extern "C" int bs_model_raster_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                   int32_t* d_model, int32_t* d_cover, int32_t* d_mz2, struct bs_model_raster* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!out)
    return fail(ctx, BS_ERR_INVALID, "model raster: null pointer");
  struct bs_model_raster res;
  memset(&res, 0, sizeof res);
  ResultGuard guard{&res};
  const int rc = raster(ctx, d_label, d_top, width, height, d_model, d_cover, d_mz2, res);
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  *out = res;
  return BS_OK;
}

extern "C" int bs_model_raster(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                               int64_t num, int64_t den, int32_t cell_log2, int32_t* model, int32_t* cover, int32_t* mz2,
                               struct bs_model_raster* out, struct bs_outline_triangles* tri, struct bs_clean_outlines* clean,
                               struct bs_simple_outlines* simple, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!label || !top || !out)
    return fail(ctx, BS_ERR_INVALID, "model raster: null pointer");
  Chain ch;
  int rc = bs_outline_triangles(ctx, label, top, width, height, n_labels, num, den, cell_log2, &ch.tri, &ch.clean, &ch.simple, &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_tri = ch.has_clean = ch.has_simple = ch.has_plain = true;
  struct bs_model_raster res;
  memset(&res, 0, sizeof res);
  ResultGuard guard{&res};
  DevBuf* B = ctx->mr;
  const size_t npix = (size_t)width * (size_t)height;
  Staging S(ctx);
  const int32_t* d_label = S.upload(B[MR_IN_LABEL], label, npix);
  const int32_t* d_top = S.upload(B[MR_IN_TOP], top, 4 * npix);
  int32_t* d_out = S.room<int32_t>(B[MR_OUT], 3 * npix);  // model | cover | mz2
  if (!S.ok())
    return S.status();
  int32_t* d_model = model ? d_out : nullptr;
  int32_t* d_cover = cover ? d_out + npix : nullptr;
  int32_t* d_mz2 = mz2 ? d_out + 2 * npix : nullptr;
  rc = raster(ctx, d_label, d_top, width, height, d_model, d_cover, d_mz2, res);
  if (rc != BS_OK)
    return rc;
  S.download(model, d_model, npix);
  S.download(cover, d_cover, npix);
  S.download(mz2, d_mz2, npix);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  ch.hand_over(tri, clean, simple, plain);
  *out = res;
  return BS_OK;
}
