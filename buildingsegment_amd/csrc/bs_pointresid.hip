// bs_pointresid.hip -- point residuals: every point of the cloud against the outline triangles (DESIGN.md "Point residuals";
// the definition is written down in include/bs_api.h under "point residuals").
//   input     bs_outline_triangles_count_dev on the context: the clean vertices with Z (bs_ctx::uc_xy, uc_z), the triangles
//             (tr_tri) and tri_offset (tr_toff) stay on the device; nothing of it is written
//   rows      per slot the pixel rows it touches (0 for a slot of -1), the range check of sz, and a record of 48 bytes: the
//             three corners, the three heights, the label; one exclusive sum: the row items.  Beside it the check of the
//             cloud, so that every BS_ERR_RANGE is known before anything is written
//   spans     per row item the pixel columns that the triangle clipped to the row's band touches, by exact integer floor and
//             ceiling; one exclusive sum: the list entries
//   lists     one thread per entry, found as the model raster finds its pixel items: a count per pixel by atomicAdd, one
//             exclusive sum, then the same pass again filling the list through a cursor per pixel
//   points    one thread per point: base pixel, its list, per entry one record and three weights with the tie rule, win and
//             cover; the winner's heights, the residual, the three outputs; the per-label figures reduced a label of the
//             wave at a time in registers, then through LDS tables below FIG_CAP and by global atomics above
// No work item's time grows with a triangle's box or area.  Every index read from memory is checked before it is used as an
// address; a violation sets err and the call returns BS_ERR_INTERNAL.
// The walk from slots to rows to spans to entries is bs_trispan.h's, shared with bs_modelraster.hip; what a span is
// (band_vertex and band_crossing, below) is this file's.
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

// scratch of bs_ctx::pr
enum { PR_MISC, PR_TMP, PR_ROWCNT, PR_ROWSCAN, PR_ROWS, PR_SPANSCAN, PR_REC, PR_CNT, PR_OFF, PR_LIST, PR_FIG, PR_PLANE, PR_IN_XYZ,
       PR_IN_PLANE, PR_OUT, PR_COUNT };
static_assert(PR_COUNT <= (int)(sizeof(bs_ctx::pr) / sizeof(DevBuf)), "bs_ctx::pr is too short");

constexpr int FIG_CAP = BS_PRESID_FIG_CAP;  // labels 0 .. FIG_CAP - 1: figures reduced in LDS (16 KiB in pr_points_kernel)
constexpr int CHUNK = BS_PRESID_CHUNK;      // list entries of one workgroup
constexpr int CHUNK_GRID = 1 << 20;         // workgroups of the list passes; beyond, a workgroup takes several chunks
constexpr int GRID = BS_PRESID_GRID;        // workgroups of the pass over the points: eight of them share a CU
constexpr long long EXTENT_LIMIT = 1ll << 24;
constexpr unsigned NO_SLOT = ~0u;
enum { W_ERR, W_RANGE, W_WORDS = 4 };                                          // the int words of PR_MISC
enum { C_UNCOVERED, C_MULTI, C_EMPTY, C_WIDE, C_MAXLIST, C_COUNT };            // its 64-bit counters, behind the words
enum { E_TRI = 1, E_ROW = 2, E_ITEM = 4, E_LIST = 8, E_WIN = 16, E_POINT = 32 };  // the bits of W_ERR
enum { R_SZ = 1, R_XY = 2, R_Z = 4 };                                          // the bits of W_RANGE
// the arrays of PR_FIG: seven counts, then the sums
enum { F_POINTS, F_MULTI, F_ABOVE, F_BELOW, F_IN, F_PPOINTS, F_PIN, F_SR, F_SABS, F_MABS, F_SQLO, F_SQHI, F_COUNT };
constexpr int N_CNT = F_PIN + 1;

// ---- 1. rows, records, and the check of the cloud ---------------------------------------------------------------------------
// (the rows of a slot: those that the triangle touches)
// record t: {a.x, a.y, b.x, b.y}, {c.x, c.y, sz[a], sz[b]}, {sz[c], label, valid, 0}
__global__ __launch_bounds__(256) void pr_rows_kernel(TriCountDev A, int32_t* __restrict__ rowcnt, int4* __restrict__ rec,
                                                      int* __restrict__ words)
{
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < A.ntri; t += (long long)gridDim.x * blockDim.x) {
    int32_t a, b, c, cnt = 0;
    int4 r0 = make_int4(0, 0, 0, 0), r1 = r0, r2 = r0;
    if (tri_of(A, t, a, b, c, words + W_ERR, E_TRI)) {
      const int32_t za = A.z[a], zb = A.z[b], zc = A.z[c];
      if (!sz_in_range(za, zb, zc))
        atomicOr(words + W_RANGE, R_SZ);
      const int2 pa = A.xy[a], pb = A.xy[b], pc = A.xy[c];
      int32_t y0, y1;
      rows_of(A.h, pa, pb, pc, y0, y1);
      cnt = max(y1 - y0, 0);
      const int32_t l = label_of_slot(A.toff, A.nl, t);
      r0 = make_int4(pa.x, pa.y, pb.x, pb.y);
      r1 = make_int4(pc.x, pc.y, za, zb);
      r2 = make_int4(zc, l, 1, 0);
    }
    rowcnt[t] = cnt;
    rec[3 * t] = r0;
    rec[3 * t + 1] = r1;
    rec[3 * t + 2] = r2;
  }
}

__global__ __launch_bounds__(256) void pr_check_kernel(const int32_t* __restrict__ xyz, long long n, int32_t bin, int32_t w, int32_t h,
                                                       int* __restrict__ words)
{
  int bad = 0;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (x < 0 || y < 0 || x / bin >= w || y / bin >= h)
      bad |= R_XY;
    if (z >= Z_LIMIT || z <= -Z_LIMIT)
      bad |= R_Z;
  }
  for (int o = 32; o > 0; o >>= 1)
    bad |= __shfl_xor(bad, o);
  if ((threadIdx.x & 63) == 0 && bad)
    atomicOr(words + W_RANGE, bad);
}

struct PixCount {  // 0 for the entry behind the last
  const unsigned* cnt;
  long long n;
  __host__ __device__ unsigned operator()(long long i) const { return i < n ? cnt[i] : 0u; }
};
using PixCountIt = hipcub::TransformInputIterator<unsigned, PixCount, Idx64>;

// ---- 2. spans -------------------------------------------------------------------------------------------------------------
// the crossing of the edge u -> v with the lattice line Y = k where that lies strictly between its ends, at
// X = u.x + num / den: its floor into lo, its ceiling into hi
__device__ inline void band_crossing(int2 u, int2 v, int32_t k, long long& lo, long long& hi)
{
  if (!((u.y < k && v.y > k) || (u.y > k && v.y < k)))
    return;
  long long den = (long long)v.y - u.y, num = ((long long)v.x - u.x) * ((long long)k - u.y);
  if (den < 0) {
    den = -den;
    num = -num;
  }
  long long q = num / den;
  const long long rem = num - q * den;
  if (rem < 0)
    q--;
  lo = min(lo, u.x + q);
  hi = max(hi, u.x + q + (rem != 0));
}

__device__ inline void band_vertex(int2 u, int32_t y, long long& lo, long long& hi)
{
  if (u.y >= y && u.y <= y + 1) {
    lo = min(lo, (long long)u.x);
    hi = max(hi, (long long)u.x);
  }
}

__global__ __launch_bounds__(256) void pr_spans_kernel(TriCountDev A, const long long* __restrict__ rowscan, long long n_rows,
                                                       int4* __restrict__ rows, int* __restrict__ words)
{
  for (long long r = blockIdx.x * (long long)blockDim.x + threadIdx.x; r < n_rows; r += (long long)gridDim.x * blockDim.x) {
    long long t;
    int2 pa, pb, pc;
    int32_t x0 = 0, len = 0, y = 0;
    if (row_of(A, rowscan, r, t, pa, pb, pc, y, words + W_ERR, E_TRI, E_ROW)) {
      // the band y <= Y <= y + 1: its vertices and the crossings of its two lines
      long long lo = LLONG_MAX, hi = LLONG_MIN;
      band_vertex(pa, y, lo, hi);
      band_vertex(pb, y, lo, hi);
      band_vertex(pc, y, lo, hi);
      for (int32_t k = y; k <= y + 1; k++) {
        band_crossing(pb, pc, k, lo, hi);
        band_crossing(pc, pa, k, lo, hi);
        band_crossing(pa, pb, k, lo, hi);
      }
      if (lo != LLONG_MAX)  // the columns floor(xmin) .. ceil(xmax) - 1
        clip_span(A.w, lo, hi - 1, x0, len);
    }
    rows[r] = make_int4((int32_t)t, y, x0, len);
  }
}

// ---- 3. lists -------------------------------------------------------------------------------------------------------------
// FILL false: cnt[p] += 1 for the pixel of every entry.  FILL true: cnt is the cursor (zeroed again), off the exclusive sum:
// the slot goes to list[off[p] + cursor++]
template <bool FILL>
__global__ __launch_bounds__(CHUNK) void pr_lists_kernel(TriCountDev A, const long long* __restrict__ spanscan,
                                                         const int4* __restrict__ rows, long long n_rows, long long n_items,
                                                         unsigned* __restrict__ cnt, const unsigned* __restrict__ off,
                                                         unsigned* __restrict__ list, int* __restrict__ err,
                                                         unsigned long long* __restrict__ counters)
{
  __shared__ long long s_row[2];  // the rows of the first and of the last entry of the chunk
  const long long n_chunks = (n_items + CHUNK - 1) / CHUNK;
  unsigned longest = 0;
  for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const long long base = chunk * CHUNK, last = min(base + CHUNK, n_items) - 1;
    if (threadIdx.x < 2)
      s_row[threadIdx.x] = last_le(spanscan, 0, n_rows - 1, threadIdx.x == 0 ? base : last);
    __syncthreads();
    const long long i = base + threadIdx.x;
    if (i <= last) {
      int32_t slot, y;
      long long x;
      if (item_of(A, spanscan, rows, s_row, i, slot, x, y, err, E_ITEM)) {
        const long long p = (long long)y * A.w + x;
        if (!FILL) {
          atomicAdd(cnt + p, 1u);
        } else {
          const unsigned k = atomicAdd(cnt + p, 1u);
          const unsigned long long at = (unsigned long long)off[p] + k;
          if (at >= off[p + 1] || at >= (unsigned long long)n_items)
            atomicOr(err, E_LIST);
          else
            list[at] = (unsigned)slot;
          longest = max(longest, k + 1);
        }
      }
    }
    __syncthreads();
  }
  if (FILL) {
    for (int o = 32; o > 0; o >>= 1)
      longest = max(longest, __shfl_xor(longest, o));
    if ((threadIdx.x & 63) == 0 && longest)
      atomicMax(counters + C_MAXLIST, (unsigned long long)longest);
  }
}

// ---- 4. points ------------------------------------------------------------------------------------------------------------
struct Fig {  // per label, device: array j starts at base + j * stride
  unsigned long long* base;
  long long stride;
  __device__ unsigned long long* at(int j, int32_t l) const { return base + j * stride + l; }
};

struct Tables {  // the figures of the labels below FIG_CAP, in LDS: 64 bytes a label
  unsigned cnt[N_CNT][FIG_CAP];
  unsigned mabs[FIG_CAP];
  unsigned long long sr[FIG_CAP], sabs[FIG_CAP], sqlo[FIG_CAP], sqhi[FIG_CAP];
};

__device__ inline void add_count(Tables& T, const Fig& f, int which, int32_t l, unsigned v)
{
  if (!v)
    return;
  if (l < FIG_CAP)
    atomicAdd(&T.cnt[which][l], v);
  else
    atomicAdd(f.at(which, l), (unsigned long long)v);
}

// (sr is the signed sum in two's complement)
__device__ inline void add_sums(Tables& T, const Fig& f, int32_t l, unsigned long long sr, unsigned long long sabs, unsigned mabs,
                                unsigned long long sqlo, unsigned long long sqhi)
{
  if (l < FIG_CAP) {
    if (sr)
      atomicAdd(&T.sr[l], sr);
    if (sabs)
      atomicAdd(&T.sabs[l], sabs);
    if (mabs)
      atomicMax(&T.mabs[l], mabs);
    if (sqlo)
      atomicAdd(&T.sqlo[l], sqlo);
    if (sqhi)
      atomicAdd(&T.sqhi[l], sqhi);
  } else {
    if (sr)
      atomicAdd(f.at(F_SR, l), sr);
    if (sabs)
      atomicAdd(f.at(F_SABS, l), sabs);
    if (mabs)
      atomicMax(f.at(F_MABS, l), (unsigned long long)mabs);
    if (sqlo)
      atomicAdd(f.at(F_SQLO, l), sqlo);
    if (sqhi)
      atomicAdd(f.at(F_SQHI, l), sqhi);
  }
}

__device__ inline bool owns(long long w, bool up) { return w > 0 || (w == 0 && up); }

// floor((4 N + D) / (2 D)) for N = wa da + wb db + wc dc with weights >= 0 of sum D > 0 and heights 0 <= d < 2^25 above the
// lowest of the three: at most 2^26 + 1.  In 64 bits where the bit lengths prove N <= D max(d) < 2^60; in 128 elsewhere, by
// long division over the 28 bits the quotient can have
__device__ inline long long half_up_quotient(long long wa, long long wb, long long wc, long long D, int32_t da, int32_t db, int32_t dc,
                                             bool& wide)
{
  const int32_t m = max(da, max(db, dc));
  wide = (64 - __clzll(D)) + (32 - __clz(m)) > 60;
  if (!wide) {
    const unsigned long long N = (unsigned long long)wa * (unsigned)da + (unsigned long long)wb * (unsigned)db +
                                 (unsigned long long)wc * (unsigned)dc;
    return (long long)((4 * N + (unsigned long long)D) / (2 * (unsigned long long)D));
  }
  typedef unsigned __int128 u128;
  const u128 N = (u128)(unsigned long long)wa * (unsigned)da + (u128)(unsigned long long)wb * (unsigned)db +
                 (u128)(unsigned long long)wc * (unsigned)dc;
  u128 rest = 4 * N + (unsigned long long)D;
  const u128 den = 2 * (u128)(unsigned long long)D;
  long long q = 0;
  for (int bit = 27; bit >= 0; bit--) {
    const u128 d = den << bit;
    if (d <= rest) {
      rest -= d;
      q |= 1ll << bit;
    }
  }
  return q;
}

__global__ __launch_bounds__(256, 8) void pr_points_kernel(const int32_t* __restrict__ xyz, long long n, int32_t bin, int32_t w, int32_t h,
                                                           long long ntri, long long n_items, int32_t nl,
                                                           const unsigned* __restrict__ off, const unsigned* __restrict__ list,
                                                           const int4* __restrict__ rec, const int32_t* __restrict__ plane_idx,
                                                           const int32_t* __restrict__ label_plane, int32_t clip2,
                                                           int32_t* __restrict__ label_out, int32_t* __restrict__ r2_out,
                                                           int32_t* __restrict__ cover_out, Fig f, int* __restrict__ words,
                                                           unsigned long long* __restrict__ counters)
{
  __shared__ Tables T;
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    for (int j = 0; j < N_CNT; j++)
      T.cnt[j][k] = 0;
    T.mabs[k] = 0;
    T.sr[k] = T.sabs[k] = T.sqlo[k] = T.sqhi[k] = 0;
  }
  __syncthreads();
  unsigned n_unc = 0, n_multi = 0, n_empty = 0, n_wide = 0;
  // (n < 2^29: 3 i, a pixel's number and every doubled coordinate fit 32 bits -- the extents are at most 2^24)
  const unsigned n64 = ((unsigned)n + 63u) & ~63u;  // whole waves stay together
  const int32_t two_bin = 2 * bin;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n64; i += gridDim.x * blockDim.x) {
    int32_t M = -1, r2 = INT32_MIN;
    unsigned cov = 0, in = 0, above = 0, below = 0, pl = 0, mabs = 0;
    unsigned long long sqlo = 0, sqhi = 0;
    if (i < (unsigned)n) {
      const int32_t x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
      const int32_t bx = x / bin, by = y / bin;
      if (x < 0 || y < 0 || bx >= w || by >= h || z >= Z_LIMIT || z <= -Z_LIMIT) {
        atomicOr(words + W_ERR, E_POINT);  // (the check pass has seen every point)
      } else {
        const unsigned p = (unsigned)by * (unsigned)w + (unsigned)bx;
        const int32_t px = 2 * x + 1, py = 2 * y + 1;
        const unsigned lo = off[p], hi = off[p + 1];
        unsigned win = NO_SLOT;
        long long wa = 0, wb = 0, wc = 0;
        if (lo > hi || hi > (unsigned long long)n_items) {
          atomicOr(words + W_ERR, E_LIST);
        } else {
          n_empty += lo == hi;
          for (unsigned k = lo; k < hi; k++) {
            const unsigned t = list[k];
            if (t >= (unsigned long long)ntri) {
              atomicOr(words + W_ERR, E_LIST);
              continue;
            }
            const int4 r0 = rec[3ll * t], r1 = rec[3ll * t + 1];
            const int32_t ax = two_bin * r0.x - px, ay = two_bin * r0.y - py, bx2 = two_bin * r0.z - px, by2 = two_bin * r0.w - py,
                          cx = two_bin * r1.x - px, cy = two_bin * r1.y - py;
            const long long ua = (long long)bx2 * cy - (long long)by2 * cx;  // orient(P, B, C), edge B -> C
            const long long ub = (long long)cx * ay - (long long)cy * ax;    // orient(P, C, A), edge C -> A
            const long long uc = (long long)ax * by2 - (long long)ay * bx2;  // orient(P, A, B), edge A -> B
            if (owns(ua, r1.y > r0.w) && owns(ub, r0.y > r1.y) && owns(uc, r0.w > r0.y)) {
              cov++;
              if (t < win) {
                win = t;
                wa = ua;
                wb = ub;
                wc = uc;
              }
            }
          }
        }
        if (win != NO_SLOT) {
          const int4 r1 = rec[3ll * win + 1], r2rec = rec[3ll * win + 2];
          const int32_t za = r1.z, zb = r1.w, zc = r2rec.x, l = r2rec.y;
          const long long D = wa + wb + wc;
          if (D <= 0 || r2rec.z != 1 || (uint32_t)l >= (uint32_t)nl) {
            atomicOr(words + W_ERR, E_WIN);
          } else {
            const int32_t zm = min(za, min(zb, zc));
            bool wide;
            const long long q = half_up_quotient(wa, wb, wc, D, za - zm, zb - zm, zc - zm, wide);
            n_wide += wide;
            M = l;
            r2 = 2 * z - (2 * zm + (int32_t)q);
            above = r2 > clip2;
            below = r2 < -clip2;
            in = !above && !below;
            if (plane_idx)
              pl = plane_idx[i] == label_plane[l];
            if (in) {
              const unsigned long long ae = (unsigned long long)(r2 < 0 ? -(long long)r2 : (long long)r2), sq = ae * ae;
              mabs = (unsigned)ae;
              sqlo = sq & 0xFFFFFFFFull;
              sqhi = sq >> 32;
            }
          }
        }
        if (label_out)
          label_out[i] = M;
        if (r2_out)
          r2_out[i] = r2;
        if (cover_out)
          cover_out[i] = (int32_t)cov;
        n_unc += M < 0;
        n_multi += M >= 0 && cov > 1;
      }
    }
    // the figures, one label of the wave at a time: the lanes of the leader's label reduce in registers and lane 0 adds
    // once (a wave inside one label takes one turn; a count of the wave is at most 64, so four of them share a word, a
    // byte each)
    const unsigned c0 = (cov > 1) | (in << 8) | (above << 16) | (below << 24), c1 = pl | ((pl & in) << 8);
    unsigned long long todo = __ballot(M >= 0);
    while (todo) {
      const int32_t Mk = __shfl(M, __ffsll(todo) - 1);
      const bool mine = M == Mk;
      const unsigned long long members = __ballot(mine);
      unsigned k0 = mine ? c0 : 0u, k1 = mine ? c1 : 0u, mx = mine ? mabs : 0u;
      unsigned long long sabs = mx, sr = mine && in ? (unsigned long long)(long long)r2 : 0ull, lo = mine ? sqlo : 0ull,
                         hi = mine ? sqhi : 0ull;
      for (int o = 32; o > 0; o >>= 1) {
        k0 += __shfl_xor(k0, o);
        k1 += __shfl_xor(k1, o);
        mx = max(mx, __shfl_xor(mx, o));
        sabs += __shfl_xor(sabs, o);
        sr += __shfl_xor(sr, o);
        lo += __shfl_xor(lo, o);
        hi += __shfl_xor(hi, o);
      }
      if ((threadIdx.x & 63) == 0) {
        add_count(T, f, F_POINTS, Mk, (unsigned)__popcll(members));
        add_count(T, f, F_MULTI, Mk, k0 & 255);
        add_count(T, f, F_IN, Mk, (k0 >> 8) & 255);
        add_count(T, f, F_ABOVE, Mk, (k0 >> 16) & 255);
        add_count(T, f, F_BELOW, Mk, k0 >> 24);
        add_count(T, f, F_PPOINTS, Mk, k1 & 255);
        add_count(T, f, F_PIN, Mk, k1 >> 8);
        add_sums(T, f, Mk, sr, sabs, mx, lo, hi);
      }
      todo &= ~members;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    n_unc += __shfl_xor(n_unc, o);
    n_multi += __shfl_xor(n_multi, o);
    n_empty += __shfl_xor(n_empty, o);
    n_wide += __shfl_xor(n_wide, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (n_unc)
      atomicAdd(counters + C_UNCOVERED, (unsigned long long)n_unc);
    if (n_multi)
      atomicAdd(counters + C_MULTI, (unsigned long long)n_multi);
    if (n_empty)
      atomicAdd(counters + C_EMPTY, (unsigned long long)n_empty);
    if (n_wide)
      atomicAdd(counters + C_WIDE, (unsigned long long)n_wide);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nl; k += blockDim.x) {
    for (int j = 0; j < N_CNT; j++)
      if (T.cnt[j][k])
        atomicAdd(f.at(j, k), (unsigned long long)T.cnt[j][k]);
    if (T.sr[k])
      atomicAdd(f.at(F_SR, k), T.sr[k]);
    if (T.sabs[k])
      atomicAdd(f.at(F_SABS, k), T.sabs[k]);
    if (T.mabs[k])
      atomicMax(f.at(F_MABS, k), (unsigned long long)T.mabs[k]);
    if (T.sqlo[k])
      atomicAdd(f.at(F_SQLO, k), T.sqlo[k]);
    if (T.sqhi[k])
      atomicAdd(f.at(F_SQHI, k), T.sqhi[k]);
  }
}

int internal(bs_ctx* ctx, int err)
{
  char msg[96];
  snprintf(msg, sizeof msg, "point residuals: an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

int range_error(bs_ctx* ctx, int bits)
{
  if (bits & R_SZ)
    return fail(ctx, BS_ERR_RANGE, "point residuals: a vertex of a triangle lies 2^24 or more above or below 0");
  if (bits & R_XY)
    return fail(ctx, BS_ERR_RANGE, "point residuals: a point with a negative x or y, or whose pixel lies outside the image");
  return fail(ctx, BS_ERR_RANGE, "point residuals: a point lies 2^24 or more above or below 0");
}

// the residuals of the device cloud against the triangle state on ctx; res is zeroed; the three outputs may be NULL;
// label_plane is a host table or NULL
int residuals(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, const int32_t* d_plane_idx, const int32_t* label_plane,
              int32_t clip2, int32_t* d_label_out, int32_t* d_r2, int32_t* d_cover, struct bs_point_residuals& res)
{
  TriCountDev A;
  int rc = tri_count_dev(ctx, "point residuals", A);
  if (rc != BS_OK)
    return rc;
  if (!d_xyz || n < 1 || bin < 1 || clip2 < 0)
    return fail(ctx, BS_ERR_INVALID, "point residuals: a null cloud, n < 1, bin < 1 or clip2 < 0");
  if ((d_plane_idx == nullptr) != (label_plane == nullptr))
    return fail(ctx, BS_ERR_INVALID, "point residuals: plane_idx and label_plane come together or not at all");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "point residuals: 2^29 points or more");
  const int32_t width = A.w, height = A.h, nl = A.nl;
  if ((long long)width * bin > EXTENT_LIMIT || (long long)height * bin > EXTENT_LIMIT)
    return fail(ctx, BS_ERR_RANGE, "point residuals: an extent (width or height times bin) above 2^24");
  const long long ntri = A.ntri, npix = (long long)width * height;
  rc = check_slots(ctx, "point residuals", A, BS_ERR_RANGE);
  if (rc != BS_OK)
    return rc;
  if (width < 1 || height < 1 || npix >= INT32_MAX || (ntri > 0 && (!A.xy || !A.z || nl < 1)))
    return internal(ctx, 0x10000);
  res.width = width;
  res.height = height;
  res.n_labels = nl;
  res.bin = bin;
  res.clip2 = clip2;
  res.fig_cap = FIG_CAP;
  res.chunk = CHUNK;
  res.grid = GRID;
  res.n_points = n;
  res.n_triangles = ctx->tr_ntri;
  const size_t nls = (size_t)std::max(nl, 0), nl1 = std::max<size_t>(nls, 1);
  int64_t** const arrays[F_COUNT] = {&res.points,       &res.multi,    &res.above,  &res.below,      &res.in_points, &res.plane_points,
                                     &res.plane_in,     &res.sum_r2,   &res.sum_abs_r2, &res.max_abs_r2, &res.sq_lo, &res.sq_hi};
  for (auto a : arrays)
    if (!alloc(a, nls))
      return fail(ctx, BS_ERR_NOMEM, "point residuals: host allocation");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->pr;
  Events<5> ev;
  for (int i = 0; i < 5; i++)
    BS_HIP(ctx, hipEventCreate(&ev.e[i]));
  const size_t fig_bytes = 8 * (size_t)F_COUNT * nl1, misc_bytes = 4 * W_WORDS + 8 * C_COUNT;
  BS_HIP(ctx, B[PR_MISC].reserve(misc_bytes));
  BS_HIP(ctx, B[PR_FIG].reserve(fig_bytes));
  BS_HIP(ctx, B[PR_PLANE].reserve(4 * nl1));
  BS_HIP(ctx, B[PR_CNT].reserve(4 * (size_t)npix));
  BS_HIP(ctx, B[PR_OFF].reserve(4 * ((size_t)npix + 1)));
  BS_HIP(ctx, B[PR_ROWCNT].reserve(4 * (size_t)std::max(ntri, 1ll)));
  BS_HIP(ctx, B[PR_ROWSCAN].reserve(8 * ((size_t)ntri + 1)));
  BS_HIP(ctx, B[PR_REC].reserve(48 * (size_t)std::max(ntri, 1ll)));
  int* d_words = B[PR_MISC].as<int>();
  unsigned long long* d_counters = reinterpret_cast<unsigned long long*>(d_words + W_WORDS);
  unsigned* cnt = B[PR_CNT].as<unsigned>();
  unsigned* off = B[PR_OFF].as<unsigned>();
  int32_t* rowcnt = B[PR_ROWCNT].as<int32_t>();
  long long* rowscan = B[PR_ROWSCAN].as<long long>();
  int4* rec = B[PR_REC].as<int4>();
  int32_t* d_label_plane = B[PR_PLANE].as<int32_t>();
  const Fig f{B[PR_FIG].as<unsigned long long>(), (long long)nl1};
  long long n_rows = 0, n_items = 0;
  int h_words[W_WORDS] = {};
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_words, 0, misc_bytes, st));
  BS_HIP(ctx, hipMemsetAsync(B[PR_FIG].p, 0, fig_bytes, st));
  BS_HIP(ctx, hipMemsetAsync(cnt, 0, 4 * (size_t)npix, st));
  if (label_plane && nls)
    BS_HIP(ctx, hipMemcpyAsync(d_label_plane, label_plane, 4 * nls, hipMemcpyHostToDevice, st));
  pr_check_kernel<<<sweep(n), 256, 0, st>>>(d_xyz, n, bin, width, height, d_words);
  if (ntri > 0) {
    // 1. rows
    pr_rows_kernel<<<sweep(ntri), 256, 0, st>>>(A, rowcnt, rec, d_words);
    BS_HIP(ctx, scan_counts(B[PR_TMP], RowCount{rowcnt, ntri}, ntri, rowscan, &n_rows, st));
  }
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_WORDS, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // n_rows, and the ranges of the cloud and of sz
  BS_HIP(ctx, hipGetLastError());
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  if (h_words[W_ERR])
    return internal(ctx, h_words[W_ERR]);
  if (h_words[W_RANGE])
    return range_error(ctx, h_words[W_RANGE]);
  if (n_rows >= INT32_MAX)
    return fail(ctx, BS_ERR_RANGE, "point residuals: 2^31 row items or more");
  const int4* rows = nullptr;
  const long long* spanscan = nullptr;
  if (n_rows > 0) {
    // 2. spans
    BS_HIP(ctx, B[PR_ROWS].reserve(16 * (size_t)n_rows));
    BS_HIP(ctx, B[PR_SPANSCAN].reserve(8 * ((size_t)n_rows + 1)));
    pr_spans_kernel<<<sweep(n_rows), 256, 0, st>>>(A, rowscan, n_rows, B[PR_ROWS].as<int4>(), d_words);
    BS_HIP(ctx, scan_counts(B[PR_TMP], SpanCount{B[PR_ROWS].as<int4>(), n_rows}, n_rows, B[PR_SPANSCAN].as<long long>(), &n_items, st));
    BS_HIP(ctx, hipStreamSynchronize(st));  // n_items
    rows = B[PR_ROWS].as<int4>();
    spanscan = B[PR_SPANSCAN].as<long long>();
  }
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  if (n_items >= INT32_MAX)
    return fail(ctx, BS_ERR_RANGE, "point residuals: 2^31 list entries or more");
  // 3. lists
  BS_HIP(ctx, B[PR_LIST].reserve(4 * (size_t)std::max(n_items, 1ll)));
  unsigned* list = B[PR_LIST].as<unsigned>();
  const long long n_chunks = (n_items + CHUNK - 1) / CHUNK;
  const int chunk_grid = (int)std::max<long long>(1, std::min<long long>(n_chunks, CHUNK_GRID));
  if (n_items > 0)
    pr_lists_kernel<false><<<chunk_grid, CHUNK, 0, st>>>(A, spanscan, rows, n_rows, n_items, cnt, off, list, d_words + W_ERR, d_counters);
  BS_HIP(ctx, cub_run(B[PR_TMP], [&](void* tmp, size_t& bytes) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, PixCountIt(Idx64(0), PixCount{cnt, npix}), off, (int)(npix + 1), st);
  }));
  if (n_items > 0) {
    BS_HIP(ctx, hipMemsetAsync(cnt, 0, 4 * (size_t)npix, st));
    pr_lists_kernel<true><<<chunk_grid, CHUNK, 0, st>>>(A, spanscan, rows, n_rows, n_items, cnt, off, list, d_words + W_ERR, d_counters);
  }
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_WORDS, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the checks of the lists, before the pass that writes
  BS_HIP(ctx, hipGetLastError());
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  if (h_words[W_ERR])
    return internal(ctx, h_words[W_ERR]);
  // 4. points
  pr_points_kernel<<<(int)std::max<long long>(1, std::min<long long>(nblk(n, 256), GRID)), 256, 0, st>>>(
      d_xyz, n, bin, width, height, ntri, n_items, nl, off, list, rec, d_plane_idx, d_label_plane, clip2, d_label_out, d_r2, d_cover, f,
      d_words, d_counters);
  unsigned long long h_counters[C_COUNT] = {};
  std::vector<unsigned long long> h_fig((size_t)F_COUNT * nl1);
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_WORDS, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_counters, d_counters, 8 * C_COUNT, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_fig.data(), B[PR_FIG].p, fig_bytes, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  if (h_words[W_ERR])
    return internal(ctx, h_words[W_ERR]);
  for (int j = 0; j < F_COUNT; j++)
    for (size_t l = 0; l < nls; l++)
      (*arrays[j])[l] = (int64_t)h_fig[(size_t)j * nl1 + l];
  for (size_t l = 0; l < nls; l++) {
    res.total_points += res.points[l];
    res.total_above += res.above[l];
    res.total_below += res.below[l];
    res.total_in_points += res.in_points[l];
    res.total_sum_r2 += res.sum_r2[l];
    res.total_sum_abs_r2 += res.sum_abs_r2[l];
    res.max_abs_r2_all = std::max(res.max_abs_r2_all, res.max_abs_r2[l]);
    res.total_sq_lo += res.sq_lo[l];
    res.total_sq_hi += res.sq_hi[l];
    res.total_plane_points += res.plane_points[l];
    res.total_plane_in += res.plane_in[l];
  }
  res.n_uncovered = (int64_t)h_counters[C_UNCOVERED];
  res.n_multi = (int64_t)h_counters[C_MULTI];
  res.n_empty_pixel = (int64_t)h_counters[C_EMPTY];
  res.n_height_wide = (int64_t)h_counters[C_WIDE];
  res.max_list = (int64_t)h_counters[C_MAXLIST];
  res.n_rows = n_rows;
  res.n_items = n_items;
  res.ms_rows = ev.ms(0, 1);
  res.ms_spans = ev.ms(1, 2);
  res.ms_lists = ev.ms(2, 3);
  res.ms_points = ev.ms(3, 4);
  return BS_OK;
}

using ResultGuard = FreeUnlessKept<struct bs_point_residuals, bs_point_residuals_free>;

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_point_residuals_free(struct bs_point_residuals* r)
{
  if (!r)
    return;
  free(r->points);
  free(r->multi);
  free(r->above);
  free(r->below);
  free(r->in_points);
  free(r->sum_r2);
  free(r->sum_abs_r2);
  free(r->max_abs_r2);
  free(r->sq_lo);
  free(r->sq_hi);
  free(r->plane_points);
  free(r->plane_in);
  memset(r, 0, sizeof *r);
}

extern "C" int bs_point_residuals_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, int32_t bin, const int32_t* d_plane_idx,
                                      const int32_t* label_plane, int32_t clip2, int32_t* d_label_out, int32_t* d_r2,
                                      int32_t* d_cover, struct bs_point_residuals* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!out)
    return fail(ctx, BS_ERR_INVALID, "point residuals: null pointer");
  struct bs_point_residuals res;
  memset(&res, 0, sizeof res);
  ResultGuard guard{&res};
  const int rc = residuals(ctx, d_xyz, n, bin, d_plane_idx, label_plane, clip2, d_label_out, d_r2, d_cover, res);
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  *out = res;
  return BS_OK;
}

extern "C" int bs_point_residuals(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height,
                                  int32_t n_labels, int64_t num, int64_t den, int32_t cell_log2, const int32_t* xyz, int64_t n,
                                  int32_t bin, const int32_t* plane_idx, const int32_t* label_plane, int32_t clip2,
                                  int32_t* label_out, int32_t* r2, int32_t* cover, struct bs_point_residuals* out,
                                  struct bs_outline_triangles* tri, struct bs_clean_outlines* clean,
                                  struct bs_simple_outlines* simple, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!label || !top || !out)
    return fail(ctx, BS_ERR_INVALID, "point residuals: null pointer");
  if (!xyz || n < 1 || bin < 1 || clip2 < 0)
    return fail(ctx, BS_ERR_INVALID, "point residuals: a null cloud, n < 1, bin < 1 or clip2 < 0");
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "point residuals: 2^29 points or more");
  Chain ch;
  int rc = bs_outline_triangles(ctx, label, top, width, height, n_labels, num, den, cell_log2, &ch.tri, &ch.clean, &ch.simple, &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_tri = ch.has_clean = ch.has_simple = ch.has_plain = true;
  struct bs_point_residuals res;
  memset(&res, 0, sizeof res);
  ResultGuard guard{&res};
  DevBuf* B = ctx->pr;
  const size_t np = (size_t)n;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(B[PR_IN_XYZ], xyz, 3 * np);
  int32_t* d_out = S.room<int32_t>(B[PR_OUT], 3 * np);  // label | r2 | cover
  const int32_t* d_plane = S.upload(B[PR_IN_PLANE], plane_idx, np);
  if (!S.ok())
    return S.status();
  int32_t* d_label_out = label_out ? d_out : nullptr;
  int32_t* d_r2 = r2 ? d_out + np : nullptr;
  int32_t* d_cover = cover ? d_out + 2 * np : nullptr;
  rc = residuals(ctx, d_xyz, n, bin, d_plane, label_plane, clip2, d_label_out, d_r2, d_cover, res);
  if (rc != BS_OK)
    return rc;
  S.download(label_out, d_label_out, np);
  S.download(r2, d_r2, np);
  S.download(cover, d_cover, np);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  ch.hand_over(tri, clean, simple, plain);
  *out = res;
  return BS_OK;
}
