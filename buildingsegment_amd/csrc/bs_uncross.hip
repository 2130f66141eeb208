// bs_uncross.hip -- the simplified outlines with every conflict between kept segments found and repaired (DESIGN.md "Clean
// outlines"; the definition is written down in include/bs_api.h under "clean outlines").
//   simplify  bs_simple_outlines_count_dev on the same images: node arrays in the rotated order, kept flags, ring figures
//   detect    once per round: the kept flags scanned and the kept nodes listed; per segment (named by its left kept node,
//             the right end across the ring's wrap) its end corners, labels and the count of the cells it touches, column
//             of cells by column; a scan; the (cell, segment) entries; a radix sort by cell; the run of every entry by two
//             binary searches; the pair tests -- a thread per entry against the entries behind it in a run of at most
//             HEAVY, a workgroup per tile of 256 entries with the tile's segments in LDS against the entries behind it in
//             longer runs; the marked segments counted
//   sweeps    with bs_set_outline_sweeps on, bs_sweep.hip marks the segments whose lens winds around a kept vertex, between
//             the pair tests and the count: its item count travels in the first read, its counts in the second
//   repair    the nodes of marked segments become active with their segment (L, R) from the scan and the list; one forced
//             round of the simplified stage's three kernels keeps every marked segment's choice
//   rings     the place of every kept vertex from the scan and the rotation, the flags, area2 over runs
// The host reads twice per detection (the entry count that sizes the sort; the marked count and the error word) and once
// for the result.  Every index read from memory is checked before it is used as an address; a violation sets err and the
// call returns BS_ERR_INTERNAL.  No kernel reads an array that a thread of the same launch writes.  Marks are plain stores
// of 1: neither the order of the entries nor a pair met in several cells shows in a result.
// The entry points own the results of the stages before through bs_chain.h's Chain (the clean outlines among them) and hand
// them over at their end; an early return frees them.  Launch sizes, events and host arrays are bs_host.h's.
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
#include "bs_segscan.h"
#include "bs_sweep.h"

namespace bs {
namespace {

// scratch of bs_ctx::uc
enum { UC_MISC, UC_TMP, UC_RLABEL, UC_KSCAN, UC_KLIST, UC_KEPT0, UC_SEGXY, UC_SEGLAB, UC_MARK, UC_CNT, UC_EOFF, UC_KEY0, UC_KEY1,
       UC_VAL0, UC_VAL1, UC_RUN, UC_AREA, UC_SOFF, UC_FXY, UC_FZ, UC_FRIGHT, UC_FRING, UC_FFLAG, UC_IN_LABEL, UC_IN_TOP,
       UC_OUT_XY, UC_OUT_Z, UC_OUT_RIGHT, UC_OUT_FLAG, UC_COUNT };
static_assert(UC_COUNT <= (int)(sizeof(bs_ctx::uc) / sizeof(DevBuf)), "bs_ctx::uc is too short");

constexpr int HEAVY = 64;          // a run of more entries is tested tile by tile
constexpr int TILE = 256;
constexpr int32_t KEPT = -1, DROPPED = -2;  // seg.x of a node that is not active (bs_simplify.hip)
constexpr unsigned F_REPAIRED = 4, F_MARKED = 8;

struct KeptFlag {  // 0 for the entry behind the last
  const int2* seg;
  int32_t N;
  __host__ __device__ int32_t operator()(int32_t q) const { return q < N && seg[q].x == KEPT; }
};

struct CellCount {  // the cell count of segment j, 0 behind the last segment
  const int32_t* cnt;
  const int32_t* nseg;
  __host__ __device__ long long operator()(int32_t j) const { return j < *nseg ? cnt[j] : 0; }  // (summed in 64 bits)
};

__global__ __launch_bounds__(256) void uncross_kept0_kernel(const int2* __restrict__ seg, int32_t N, uint8_t* __restrict__ kept0)
{
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x)
    kept0[q] = seg[q].x == KEPT;
}

// ---- detect ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uncross_list_kernel(const int2* __restrict__ seg, const int32_t* __restrict__ kscan, int32_t N,
                                                           int32_t* __restrict__ klist, int* __restrict__ err)
{
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
    if (seg[q].x != KEPT)
      continue;
    const int32_t j = kscan[q];
    if ((uint32_t)j >= (uint32_t)N)
      atomicOr(err, 1);
    else
      klist[j] = (int32_t)q;
  }
}

// The cells a closed segment touches, column of cells by column: in the column cx the segment covers the X from
// xa = max(x0, cx << k) to xb = min(x1, (cx + 1) << k) (x0 <= x1), and there the rows of floor(Y(xa)) and floor(Y(xb)) and
// all between.  A common point of two segments lies in one cell, and both reach it.
template <class Emit>
__device__ inline int32_t walk_cells(int4 s, int k, Emit emit)
{
  if (s.x > s.z)
    s = make_int4(s.z, s.w, s.x, s.y);
  const long long x0 = s.x, y0 = s.y, dx = s.z - s.x, dy = s.w - s.y;
  int32_t n = 0;
  for (long long cx = x0 >> k; cx <= (s.z >> k); cx++) {
    long long lo, hi;
    if (dx == 0) {
      lo = min(s.y, s.w);
      hi = max(s.y, s.w);
    } else {
      const long long xa = max(x0, cx << k), xb = min((long long)s.z, (cx + 1) << k);
      const long long fa = (y0 * dx + (xa - x0) * dy) / dx, fb = (y0 * dx + (xb - x0) * dy) / dx;  // (Y >= 0: floors)
      lo = min(fa, fb);
      hi = max(fa, fb);
    }
    for (long long cy = lo >> k; cy <= (hi >> k); cy++, n++)
      emit((int32_t)cx, (int32_t)cy, n);
  }
  return n;
}

// the right end of the segment that the kept node L of ring [r0, r1) starts, L the kept node number j
__device__ inline int32_t right_end(const int32_t* __restrict__ kscan, const int32_t* __restrict__ klist, int32_t j, int32_t r0,
                                    int32_t r1)
{
  return j + 1 < kscan[r1] ? klist[j + 1] : r0;
}

__global__ __launch_bounds__(256) void uncross_segments_kernel(const int32_t* __restrict__ kscan, const int32_t* __restrict__ klist,
                                                               const int2* __restrict__ xy, const int32_t* __restrict__ right,
                                                               const int32_t* __restrict__ ring, const int32_t* __restrict__ noff,
                                                               const int32_t* __restrict__ rlabel, int32_t N, int32_t nr, int k,
                                                               int4* __restrict__ segxy, int2* __restrict__ seglab,
                                                               uint8_t* __restrict__ mark, int32_t* __restrict__ cnt,
                                                               int* __restrict__ err)
{
  const int32_t nseg = kscan[N];
  if (nseg < 0 || nseg > N) {
    atomicOr(err, 2);
    return;
  }
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nseg; j += (int64_t)gridDim.x * blockDim.x) {
    int4 s = make_int4(0, 0, 0, 0);
    int2 lab = make_int2(-1, -1);
    int32_t c = 0;
    const int32_t L = klist[j];
    const int32_t r = (uint32_t)L < (uint32_t)N ? ring[L] : -1;
    if ((uint32_t)r >= (uint32_t)nr) {
      atomicOr(err, 2);
    } else {
      const int32_t r0 = noff[r], r1 = noff[r + 1];
      if (r0 < 0 || r0 > L || r1 <= L || r1 > N) {
        atomicOr(err, 2);
      } else {
        const int32_t R = right_end(kscan, klist, (int32_t)j, r0, r1);
        if ((uint32_t)R >= (uint32_t)N) {
          atomicOr(err, 2);
        } else {
          const int2 a = xy[L], b = xy[R];
          s = make_int4(a.x, a.y, b.x, b.y);
          lab = make_int2(rlabel[r], right[L]);
          if (min(min(a.x, a.y), min(b.x, b.y)) < 0)
            atomicOr(err, 2);
          else
            c = walk_cells(s, k, [](int32_t, int32_t, int32_t) {});
        }
      }
    }
    segxy[j] = s;
    seglab[j] = lab;
    mark[j] = 0;
    cnt[j] = c;
  }
}

__global__ __launch_bounds__(256) void uncross_fill_kernel(const int4* __restrict__ segxy, const int32_t* __restrict__ cnt,
                                                           const long long* __restrict__ eoff, int32_t nseg, int32_t E, int k,
                                                           uint32_t ncx, uint32_t* __restrict__ key, int32_t* __restrict__ val,
                                                           int* __restrict__ err)
{
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < nseg; j += (int64_t)gridDim.x * blockDim.x) {
    const long long b64 = eoff[j];
    const int32_t base = (int32_t)b64, c = cnt[j];
    if (b64 < 0 || c < 0 || b64 + c > E) {
      atomicOr(err, 4);
      continue;
    }
    if (c > 0)
      walk_cells(segxy[j], k, [=](int32_t cx, int32_t cy, int32_t i) {
        if (i < c) {
          key[base + i] = (uint32_t)cy * ncx + (uint32_t)cx;
          val[base + i] = (int32_t)j;
        }
      });
  }
}

// the run [first, behind the last) of the entries of every entry's cell in the sorted order; the longest run
__global__ __launch_bounds__(256) void uncross_runs_kernel(const uint32_t* __restrict__ key, const int32_t* __restrict__ val, int32_t E,
                                                           int32_t nseg, int2* __restrict__ run, int* __restrict__ max_cell,
                                                           int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int64_t E64 = ((int64_t)E + 63) & ~(int64_t)63;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E64; e += (int64_t)gridDim.x * blockDim.x) {
    int len = 0;
    if (e < E) {
      const uint32_t c = key[e];
      int32_t lo = 0, hi = (int32_t)e;  // the first entry with key >= c
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < c)
          lo = mid + 1;
        else
          hi = mid;
      }
      const int32_t first = lo;
      lo = (int32_t)e + 1, hi = E;  // the first entry with key > c
      while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] <= c)
          lo = mid + 1;
        else
          hi = mid;
      }
      run[e] = make_int2(first, lo);
      len = lo - first;
      if ((uint32_t)val[e] >= (uint32_t)nseg)
        atomicOr(err, 8);
    }
    for (int o = 32; o > 0; o >>= 1)
      len = max(len, __shfl_down(len, o));
    if (lane == 0 && len > 0)
      atomicMax(max_cell, len);
  }
}

__device__ inline long long orient(int ax, int ay, int bx, int by, int px, int py)
{
  return (long long)(bx - ax) * (py - ay) - (long long)(by - ay) * (px - ax);
}

// p = (px, py) with orient(u, v, p) = 0 lies on the closed segment u-v and is neither u nor v
__device__ inline bool inside_open(int ux, int uy, int vx, int vy, int px, int py)
{
  return px >= min(ux, vx) && px <= max(ux, vx) && py >= min(uy, vy) && py <= max(uy, vy) && !(px == ux && py == uy) &&
         !(px == vx && py == vy);
}

__device__ inline unsigned long long lex(int x, int y) { return ((unsigned long long)(uint32_t)x << 32) | (uint32_t)y; }

// a = (x0, y0, x1, y1) with labels (left, right); twins never conflict
__device__ inline bool conflict(int4 a, int2 al, int4 b, int2 bl)
{
  if (a.x == b.z && a.y == b.w && a.z == b.x && a.w == b.y && al.x == bl.y && al.y == bl.x)
    return false;
  if (max(a.x, a.z) < min(b.x, b.z) || max(b.x, b.z) < min(a.x, a.z) || max(a.y, a.w) < min(b.y, b.w) ||
      max(b.y, b.w) < min(a.y, a.w))
    return false;
  const long long d1 = orient(b.x, b.y, b.z, b.w, a.x, a.y), d2 = orient(b.x, b.y, b.z, b.w, a.z, a.w);
  const long long d3 = orient(a.x, a.y, a.z, a.w, b.x, b.y), d4 = orient(a.x, a.y, a.z, a.w, b.z, b.w);
  if (((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0)))
    return true;
  if (d1 == 0 && d2 == 0 && d3 == 0 && d4 == 0) {  // collinear: more than a point in common
    const unsigned long long a0 = lex(a.x, a.y), a1 = lex(a.z, a.w), b0 = lex(b.x, b.y), b1 = lex(b.z, b.w);
    return max(min(a0, a1), min(b0, b1)) < min(max(a0, a1), max(b0, b1));
  }
  return (d1 == 0 && inside_open(b.x, b.y, b.z, b.w, a.x, a.y)) || (d2 == 0 && inside_open(b.x, b.y, b.z, b.w, a.z, a.w)) ||
         (d3 == 0 && inside_open(a.x, a.y, a.z, a.w, b.x, b.y)) || (d4 == 0 && inside_open(a.x, a.y, a.z, a.w, b.z, b.w));
}

// runs of at most HEAVY entries: every entry against the entries behind it in its run
__global__ __launch_bounds__(256) void uncross_pairs_light_kernel(const int2* __restrict__ run, const int32_t* __restrict__ val,
                                                                  const int4* __restrict__ segxy, const int2* __restrict__ seglab,
                                                                  int32_t E, int32_t nseg, uint8_t* __restrict__ mark,
                                                                  int* __restrict__ err)
{
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    const int2 r = run[e];
    if (r.y - r.x > HEAVY || r.y - e < 2)
      continue;
    const int32_t ja = val[e];
    if (r.y > E || (uint32_t)ja >= (uint32_t)nseg) {
      atomicOr(err, 16);
      continue;
    }
    const int4 a = segxy[ja];
    const int2 al = seglab[ja];
    bool hit = false;
    for (int32_t p = (int32_t)e + 1; p < r.y; p++) {
      const int32_t jb = val[p];
      if ((uint32_t)jb >= (uint32_t)nseg) {
        atomicOr(err, 16);
      } else if (conflict(a, al, segxy[jb], seglab[jb])) {
        mark[jb] = 1;
        hit = true;
      }
    }
    if (hit)
      mark[ja] = 1;
  }
}

// Longer runs: a workgroup takes a tile of 256 entries of the sorted order with their segments in LDS; its threads stride
// over the entries behind the tile's first up to the end of the last long run the tile reaches, each against the entries of
// the tile that lie in its own run and in front of it.  A run of M entries is M / 256 work items of at most 256 * M tests.
__global__ __launch_bounds__(256) void uncross_pairs_heavy_kernel(const int2* __restrict__ run, const int32_t* __restrict__ val,
                                                                  const int4* __restrict__ segxy, const int2* __restrict__ seglab,
                                                                  int32_t E, int32_t nseg, uint8_t* __restrict__ mark,
                                                                  int* __restrict__ err)
{
  __shared__ int4 txy[TILE];
  __shared__ int2 tlab[TILE];
  __shared__ int32_t tseg[TILE];
  __shared__ int s_end;
  const int tid = threadIdx.x;
  const int32_t ntiles = (E + TILE - 1) / TILE;
  for (int32_t T = blockIdx.x; T < ntiles; T += gridDim.x) {
    const int32_t base = T * TILE, e = base + tid;
    if (tid == 0)
      s_end = 0;
    __syncthreads();
    int32_t my_end = 0, j = -1;
    if (e < E) {
      const int2 r = run[e];
      j = val[e];
      if ((uint32_t)j >= (uint32_t)nseg) {
        atomicOr(err, 32);
        j = -1;
      } else {
        txy[tid] = segxy[j];
        tlab[tid] = seglab[j];
        if (r.y - r.x > HEAVY)
          my_end = min(r.y, E);
      }
    }
    tseg[tid] = j;
    if (my_end > 0)
      atomicMax(&s_end, my_end);
    __syncthreads();
    const int32_t end = s_end;
    for (int32_t p = base + 1 + tid; p < end; p += TILE) {
      const int2 r = run[p];
      if (r.y - r.x <= HEAVY)
        continue;
      const int32_t lo = max(base, r.x), hi = min(base + TILE, p);
      const int32_t jb = val[p];
      if ((uint32_t)jb >= (uint32_t)nseg) {
        atomicOr(err, 32);
        continue;
      }
      const int4 b = segxy[jb];
      const int2 bl = seglab[jb];
      bool hit = false;
      for (int32_t i = lo; i < hi; i++) {
        const int32_t ja = tseg[i - base];
        if (ja >= 0 && conflict(txy[i - base], tlab[i - base], b, bl)) {
          mark[ja] = 1;
          hit = true;
        }
      }
      if (hit)
        mark[jb] = 1;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void uncross_count_kernel(const uint8_t* __restrict__ mark, int32_t nseg, int* __restrict__ marked)
{
  const int lane = threadIdx.x & 63;
  const int64_t n64 = ((int64_t)nseg + 63) & ~(int64_t)63;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n64; j += (int64_t)gridDim.x * blockDim.x) {
    int m = j < nseg ? mark[j] : 0;
    for (int o = 32; o > 0; o >>= 1)
      m += __shfl_down(m, o);
    if (lane == 0 && m > 0)
      atomicAdd(marked, m);
  }
}

// ---- repair ----------------------------------------------------------------------------------------------------------------
// A kept node stays kept and carries its segment's mark as the forced word; a dropped node of a marked segment becomes
// active with the segment (L, R) that spans it: L is the kept node number (kept nodes in front of it) - 1.
__global__ __launch_bounds__(256) void uncross_spans_kernel(const int2* __restrict__ seg, const int32_t* __restrict__ kscan,
                                                            const int32_t* __restrict__ klist, const uint8_t* __restrict__ mark,
                                                            const int32_t* __restrict__ ring, const int32_t* __restrict__ noff,
                                                            int32_t N, int32_t nr, int2* __restrict__ seg2,
                                                            unsigned long long* __restrict__ best, unsigned long long* __restrict__ tie,
                                                            uint8_t* __restrict__ forced, int* __restrict__ err)
{
  const int32_t nseg = kscan[N];
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
    int2 s = make_int2(DROPPED, 0);
    uint8_t f = 0;
    const int32_t k = kscan[q], r = ring[q];
    if (seg[q].x == KEPT) {
      s.x = KEPT;
      if ((uint32_t)k >= (uint32_t)nseg)
        atomicOr(err, 64);
      else
        f = mark[k];
    } else if (k < 1 || k > nseg || (uint32_t)r >= (uint32_t)nr) {
      atomicOr(err, 64);
    } else if (mark[k - 1]) {
      const int32_t r0 = noff[r], r1 = noff[r + 1], L = klist[k - 1];
      if (r0 < 0 || r0 > q || r1 <= q || r1 > N || L < r0 || L >= q) {
        atomicOr(err, 64);
      } else {
        const int32_t R = right_end(kscan, klist, k - 1, r0, r1);
        if ((uint32_t)R >= (uint32_t)N)
          atomicOr(err, 64);
        else
          s = make_int2(L, R);
      }
    }
    seg2[q] = s;
    best[q] = 0;
    tie[q] = ~0ull;
    forced[q] = f;
  }
}

// ---- rings -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void uncross_offsets_kernel(const int32_t* __restrict__ kscan, const int32_t* __restrict__ noff,
                                                              int32_t nr, int32_t N, int32_t* __restrict__ soff,
                                                              unsigned long long* __restrict__ area2, int* __restrict__ err)
{
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r <= nr; r += (int64_t)gridDim.x * blockDim.x) {
    const int32_t o = noff[r];
    if ((uint32_t)o > (uint32_t)N) {
      atomicOr(err, 128);
      soff[r] = 0;
    } else {
      soff[r] = kscan[o];
    }
    if (r < nr)
      area2[r] = 0;
  }
}

struct FinalArrays {
  int2* xy;
  int32_t* z;
  int32_t* right;
  int32_t* ring;
  uint8_t* flag;
};

// the place of a kept node as in the simplified stage: its number among the kept nodes of its ring in the rotated order,
// minus the kept nodes in front of h0's place there, modulo the ring's kept count
__global__ __launch_bounds__(256) void uncross_final_kernel(const int2* __restrict__ seg, const int32_t* __restrict__ kscan,
                                                            const uint8_t* __restrict__ kept0, const uint8_t* __restrict__ mark,
                                                            const uint8_t* __restrict__ smark, const int2* __restrict__ xy,
                                                            const int32_t* __restrict__ z,
                                                            const int32_t* __restrict__ right, const int32_t* __restrict__ ring,
                                                            const uint8_t* __restrict__ flag, const int32_t* __restrict__ noff,
                                                            const int32_t* __restrict__ rot_of, int32_t N, int32_t nr, bool has_z,
                                                            FinalArrays O, int* __restrict__ err)
{
  const int32_t nseg = kscan[N];
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
    if (seg[q].x != KEPT)
      continue;
    const int32_t r = ring[q], k = kscan[q];
    if ((uint32_t)r >= (uint32_t)nr || (uint32_t)k >= (uint32_t)nseg) {
      atomicOr(err, 256);
      continue;
    }
    const int32_t r0 = noff[r], r1 = noff[r + 1], rot = rot_of[r];
    if (r0 < 0 || r0 > q || r1 <= q || r1 > N || rot < 0 || rot >= r1 - r0) {
      atomicOr(err, 256);
      continue;
    }
    const int32_t s0 = kscan[r0], kc = kscan[r1] - s0, kb = kscan[r1 - rot] - s0;
    int32_t o = k - s0 - kb;
    if (o < 0)
      o += kc;
    const int64_t d = (int64_t)s0 + o;
    if (o < 0 || o >= kc || d < 0 || d >= N) {
      atomicOr(err, 256);
      continue;
    }
    O.xy[d] = xy[q];
    O.right[d] = right[q];
    O.ring[d] = r;
    const unsigned sm = smark ? smark[k] : 0u;  // (sweeps on: a mark that only a sweep set is no conflict)
    O.flag[d] = (uint8_t)((flag[q] & 3u) | (kept0[q] ? 0u : F_REPAIRED) | (mark[k] && !(sm & SM_ONLY) ? F_MARKED : 0u) |
                          (sm & SM_SWEEPING ? F_SWEEPING : 0u));
    if (has_z)
      O.z[d] = z[q];
  }
}

__global__ __launch_bounds__(256) void uncross_area_kernel(const int2* __restrict__ xy, const int32_t* __restrict__ ring,
                                                           const int32_t* __restrict__ soff, const int32_t* __restrict__ kscan,
                                                           int32_t N, int32_t nr, unsigned long long* __restrict__ area2,
                                                           int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int32_t nsv = kscan[N];
  if (nsv < 0 || nsv > N) {
    atomicOr(err, 512);
    return;
  }
  const int64_t n64 = ((int64_t)nsv + 63) & ~(int64_t)63;
  for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < n64; d += (int64_t)gridDim.x * blockDim.x) {
    int32_t r = -1;
    long long term = 0;
    if (d < nsv) {
      r = ring[d];
      if ((uint32_t)r >= (uint32_t)nr) {
        atomicOr(err, 512);
        r = -1;
      } else {
        const int32_t a = soff[r], b = soff[r + 1];
        if (a < 0 || a > d || b <= d || b > nsv) {
          atomicOr(err, 512);
          r = -1;
        } else {
          const int2 u = xy[d], v = xy[d + 1 < b ? d + 1 : a];
          term = (long long)u.x * v.y - (long long)v.x * u.y;
        }
      }
    }
    const int32_t prev = __shfl_up(r, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != r);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    BS_SEG_SCAN(term, BS_OP_ADD)
    if (lane == tl && r >= 0)
      atomicAdd(area2 + r, (unsigned long long)term);
  }
}

__global__ __launch_bounds__(256) void uncross_emit_kernel(FinalArrays O, int64_t nsv, int2* __restrict__ xy, int32_t* __restrict__ z,
                                                           int32_t* __restrict__ right, uint8_t* __restrict__ flag)
{
  for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < nsv; d += (int64_t)gridDim.x * blockDim.x) {
    xy[d] = O.xy[d];
    right[d] = O.right[d];
    flag[d] = O.flag[d];
    if (z)
      z[d] = O.z[d];
  }
}

int internal(bs_ctx* ctx, int err)
{
  char msg[96];
  snprintf(msg, sizeof msg, "clean outlines: an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

FinalArrays final_arrays(DevBuf* B)
{
  return FinalArrays{B[UC_FXY].as<int2>(), B[UC_FZ].as<int32_t>(), B[UC_FRIGHT].as<int32_t>(), B[UC_FRING].as<int32_t>(),
                     B[UC_FFLAG].as<uint8_t>()};
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_clean_outlines_free(struct bs_clean_outlines* s)
{
  if (!s)
    return;
  free(s->ring_label);
  free(s->ring_area2);
  free(s->label_ring_offset);
  free(s->s_ring_vertices);
  free(s->s_ring_area2);
  free(s->s_ring_arcs);
  free(s->s_ring_offset);
  free(s->sxy);
  free(s->sz);
  free(s->s_right);
  free(s->s_flag);
  memset(s, 0, sizeof *s);
}

extern "C" int bs_clean_outlines_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                           int32_t n_labels, int64_t num, int64_t den, int32_t max_rounds, int32_t cell_log2,
                                           struct bs_clean_outlines* out, struct bs_simple_outlines* simple,
                                           struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->uc_valid = false;
  ctx->ps_valid = false;  // (the polygon solids' emit reads the clean vertices)
  if (!out || cell_log2 < 0 || cell_log2 > 30)
    return fail(ctx, BS_ERR_INVALID, "clean outlines: null pointer or cell_log2 outside 0 .. 30");
  Chain ch;  // (its clean outlines are this call's own result)
  struct bs_simple_outlines& sm = ch.simple;
  struct bs_clean_outlines& res = ch.clean;
  int rc = bs_simple_outlines_count_dev(ctx, d_label, d_top, width, height, n_labels, num, den, &sm, &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_plain = ch.has_simple = ch.has_clean = true;
  const int mode = ctx->sweeps_mode;
  struct bs_outline_sweeps sw;
  memset(&sw, 0, sizeof sw);
  sw.mode = mode;
  sw.wave_cap = BS_SWEEP_WAVE_CAP;
  const int k = cell_log2 == 0 ? BS_CLEAN_DEFAULT_CELL_LOG2 : cell_log2;
  const int32_t nr = (int32_t)sm.n_rings;
  const bool has_z = d_top != nullptr;
  res.width = width;
  res.height = height;
  res.n_labels = n_labels;
  res.has_z = has_z;
  res.tol_num = sm.tol_num;
  res.tol_den = sm.tol_den;
  res.max_rounds = max_rounds;
  res.cell_log2 = k;
  res.n_rings = nr;
  res.n_nodes = sm.n_nodes;
  res.n_junction_nodes = sm.n_junction_nodes;
  res.n_arcs = sm.n_arcs;
  res.rounds = sm.rounds;
  res.max_arc_nodes = sm.max_arc_nodes;
  res.n_svertices = res.n_svertices_before = sm.n_svertices;
  res.ms_simplify = sm.ms_outlines + sm.ms_nodes + sm.ms_placing + sm.ms_arcs + sm.ms_rounds + sm.ms_rings;
  const bool ok[] = {alloc(&res.ring_label, nr),      alloc(&res.ring_area2, nr),  alloc(&res.label_ring_offset, (size_t)n_labels + 1),
                     alloc(&res.s_ring_vertices, nr), alloc(&res.s_ring_area2, nr), alloc(&res.s_ring_arcs, nr),
                     alloc(&res.s_ring_offset, (size_t)nr + 1)};
  if (!std::all_of(std::begin(ok), std::end(ok), [](bool b) { return b; }))
    return fail(ctx, BS_ERR_NOMEM, "clean outlines: host allocation");
  memcpy(res.label_ring_offset, sm.label_ring_offset, 8 * ((size_t)n_labels + 1));
  if (nr > 0) {
    memcpy(res.ring_label, sm.ring_label, 4 * (size_t)nr);
    memcpy(res.ring_area2, sm.ring_area2, 8 * (size_t)nr);
    memcpy(res.s_ring_arcs, sm.s_ring_arcs, 8 * (size_t)nr);
  }
  auto hand_over = [&]() {
    ctx->uc_nsv = res.n_svertices;
    ch.hand_over(nullptr, out, simple, plain);
    ctx->uc_has_z = has_z;
    ctx->uc_xy = ctx->uc[UC_FXY].as<int2>();  // (for bs_triangulate.hip)
    ctx->uc_ring = ctx->uc[UC_FRING].as<int32_t>();
    ctx->uc_soff = ctx->uc[UC_SOFF].as<int32_t>();
    ctx->uc_z = ctx->uc[UC_FZ].as<int32_t>();  // (for bs_polysolid.hip)
    ctx->uc_right = ctx->uc[UC_FRIGHT].as<int32_t>();
    ctx->uc_valid = true;
    ctx->sweeps = sw;
    return BS_OK;
  };
  const bs_ctx::SimplifyState S = ctx->sp_state;
  const int32_t N = S.N;
  if (sm.n_nodes == 0)  // no labelled pixel
    return hand_over();
  if (N != sm.n_nodes || S.nr != nr || N < 1)
    return internal(ctx, 0x10000);
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->uc;
  Events<10> ev;
  for (int i = 0; i < (mode ? 10 : 6); i++)
    BS_HIP(ctx, hipEventCreate(&ev.e[i]));
  BS_HIP(ctx, B[UC_MISC].reserve(256));
  BS_HIP(ctx, B[UC_RLABEL].reserve(4 * (size_t)nr));
  BS_HIP(ctx, B[UC_KSCAN].reserve(4 * ((size_t)N + 1)));
  BS_HIP(ctx, B[UC_EOFF].reserve(8 * ((size_t)N + 1)));
  for (int b : {UC_KLIST, UC_CNT, UC_FZ, UC_FRIGHT, UC_FRING})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)N));
  for (int b : {UC_KEPT0, UC_MARK, UC_FFLAG})
    BS_HIP(ctx, B[b].reserve((size_t)N));
  BS_HIP(ctx, B[UC_SEGXY].reserve(16 * (size_t)N));
  for (int b : {UC_SEGLAB, UC_FXY})
    BS_HIP(ctx, B[b].reserve(8 * (size_t)N));
  BS_HIP(ctx, B[UC_AREA].reserve(8 * (size_t)nr));
  BS_HIP(ctx, B[UC_SOFF].reserve(4 * ((size_t)nr + 1)));
  int* d_words = B[UC_MISC].as<int>();
  int* d_err = d_words + W_ERR;
  int32_t* rlabel = B[UC_RLABEL].as<int32_t>();
  int32_t* kscan = B[UC_KSCAN].as<int32_t>();
  long long* eoff = B[UC_EOFF].as<long long>();
  int32_t* klist = B[UC_KLIST].as<int32_t>();
  int32_t* cnt = B[UC_CNT].as<int32_t>();
  uint8_t* kept0 = B[UC_KEPT0].as<uint8_t>();
  uint8_t* mark = B[UC_MARK].as<uint8_t>();
  int4* segxy = B[UC_SEGXY].as<int4>();
  int2* seglab = B[UC_SEGLAB].as<int2>();
  unsigned long long* area2 = B[UC_AREA].as<unsigned long long>();
  int32_t* soff = B[UC_SOFF].as<int32_t>();
  const FinalArrays O = final_arrays(B);
  int2* segK = S.seg[S.cur];      // holds the kept flags
  int2* segW = S.seg[S.cur ^ 1];  // the active nodes of a repair round
  hipcub::CountingInputIterator<int32_t> idx(0);
  hipcub::TransformInputIterator<int32_t, KeptFlag, hipcub::CountingInputIterator<int32_t>> kf(idx, KeptFlag{segK, N});
  hipcub::TransformInputIterator<long long, CellCount, hipcub::CountingInputIterator<int32_t>> cc(idx, CellCount{cnt, kscan + N});
  auto scan_kept = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, kf, kscan, N + 1, st); };
  auto scan_cells = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, cc, eoff, N + 1, st); };
  BS_HIP(ctx, cub_room(B[UC_TMP], scan_kept, scan_cells));
  const uint32_t ncx = ((uint32_t)width >> k) + 1, ncy = ((uint32_t)height >> k) + 1;
  const int key_bits = bits_of((int64_t)ncx * ncy);
  const int g = sweep(N);
  BS_HIP(ctx, hipMemsetAsync(d_words, 0, 4 * W_COUNT, st));
  BS_HIP(ctx, hipMemcpyAsync(rlabel, sm.ring_label, 4 * (size_t)nr, hipMemcpyHostToDevice, st));
  uncross_kept0_kernel<<<g, 256, 0, st>>>(segK, N, kept0);
  int64_t rounds = 0;
  double ms_detect = 0, ms_repair = 0;
  const SweepRun SR{st, segK, kscan, klist, S.xy, S.ring, S.noff, N, nr, width, height, d_words, mode};
  bool repair_pending = false;
  int h_words[W_COUNT] = {};
  for (;;) {
    // ---- detect ----
    BS_HIP(ctx, hipEventRecord(ev.e[0], st));
    BS_HIP(ctx, cub_run(B[UC_TMP], scan_kept));
    uncross_list_kernel<<<g, 256, 0, st>>>(segK, kscan, N, klist, d_err);
    uncross_segments_kernel<<<g, 256, 0, st>>>(kscan, klist, S.xy, S.right, S.ring, S.noff, rlabel, N, nr, k, segxy, seglab, mark, cnt,
                                               d_err);
    BS_HIP(ctx, cub_run(B[UC_TMP], scan_cells));
    long long E64 = 0, I64 = 0;
    if (mode) {  // the sweep pass's items: counted here, so that their count travels in the first read
      BS_HIP(ctx, hipEventRecord(ev.e[6], st));
      if (int rcs = sweep_begin(ctx, SR, &I64))
        return rcs;
      BS_HIP(ctx, hipEventRecord(ev.e[7], st));
    }
    int32_t nseg = 0;
    int h_err = 0;
    BS_HIP(ctx, hipMemcpyAsync(&E64, eoff + N, 8, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(&nseg, kscan + N, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));  // the entry count sizes the sort
    BS_HIP(ctx, hipGetLastError());
    if (h_err)
      return internal(ctx, h_err);
    if (repair_pending)  // (the repair round in front of this detection has ended with it)
      ms_repair += ev.ms(4, 5), repair_pending = false;
    if (nseg < 1 || nseg > N || E64 < nseg)
      return internal(ctx, 0x20000);
    if (E64 > INT32_MAX)
      return fail(ctx, BS_ERR_INVALID, "clean outlines: more than 2^31 - 1 (cell, segment) entries: take a larger cell_log2");
    if (I64 < 0)
      return internal(ctx, 0x200000);
    if (I64 > INT32_MAX)
      return fail(ctx, BS_ERR_INVALID, "clean outlines: more than 2^31 - 1 items of the sweep pass");
    const int32_t E = (int32_t)E64;
    for (int b : {UC_KEY0, UC_KEY1, UC_VAL0, UC_VAL1})
      BS_HIP(ctx, B[b].reserve(4 * (size_t)E));
    BS_HIP(ctx, B[UC_RUN].reserve(8 * (size_t)E));
    uint32_t* key0 = B[UC_KEY0].as<uint32_t>();
    uint32_t* key1 = B[UC_KEY1].as<uint32_t>();
    int32_t* val0 = B[UC_VAL0].as<int32_t>();
    int32_t* val1 = B[UC_VAL1].as<int32_t>();
    int2* run = B[UC_RUN].as<int2>();
    auto sort = [&](void* tmp, size_t& bytes) {
      return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, key0, key1, val0, val1, E, 0, key_bits, st);
    };
    BS_HIP(ctx, cub_room(B[UC_TMP], sort));
    uncross_fill_kernel<<<sweep(nseg), 256, 0, st>>>(segxy, cnt, eoff, nseg, E, k, ncx, key0, val0, d_err);
    BS_HIP(ctx, cub_run(B[UC_TMP], sort));
    uncross_runs_kernel<<<sweep(E), 256, 0, st>>>(key1, val1, E, nseg, run, d_words + W_MAXCELL, d_err);
    uncross_pairs_light_kernel<<<sweep(E), 256, 0, st>>>(run, val1, segxy, seglab, E, nseg, mark, d_err);
    uncross_pairs_heavy_kernel<<<sweep(E), 256, 0, st>>>(run, val1, segxy, seglab, E, nseg, mark, d_err);
    if (mode) {
      BS_HIP(ctx, hipEventRecord(ev.e[8], st));
      if (int rcs = sweep_detect(ctx, SR, nseg, I64, mark))
        return rcs;
      BS_HIP(ctx, hipEventRecord(ev.e[9], st));
    }
    BS_HIP(ctx, hipMemsetAsync(d_words + W_MARKED, 0, 4, st));
    uncross_count_kernel<<<sweep(nseg), 256, 0, st>>>(mark, nseg, d_words + W_MARKED);
    BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_COUNT, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipEventRecord(ev.e[1], st));
    BS_HIP(ctx, hipStreamSynchronize(st));  // the marked count and the error word
    BS_HIP(ctx, hipGetLastError());
    ms_detect += ev.ms(0, 1);
    if (h_words[W_ERR])
      return internal(ctx, h_words[W_ERR]);
    // (mode 2: the count is over conflicting and sweeping segments; n_marked_* are the conflicting ones)
    const int n_conflicting = h_words[W_MARKED] - (mode == 2 ? h_words[W_S_ONLY] : 0);
    if (mode) {
      sw.ms_sweep += ev.ms(6, 7) + ev.ms(8, 9);
      if (rounds == 0) {
        sw.n_lens_segments_first = h_words[W_S_LENS];
        sw.n_sweeping_first = h_words[W_S_SWEEPING];
        sw.n_sweeping_only_first = h_words[W_S_ONLY];
        sw.n_swept_pairs_first = h_words[W_S_PAIRS];
        sw.n_items_first = I64;
        sw.n_items_swapped_first = h_words[W_S_ITEMS_T];
        sw.n_candidates_first =
            (long long)(((unsigned long long)(uint32_t)h_words[W_S_CAND_HI] << 32) | (uint32_t)h_words[W_S_CAND_LO]);
        sw.n_exact_first = h_words[W_S_EXACT];
        sw.n_exact_wave_first = h_words[W_S_WAVE];
        sw.n_rejected_first = h_words[W_S_REJECT];
      }
      sw.max_abs_winding = h_words[W_S_MAXW];
      sw.n_sweeping_left = h_words[W_S_SWEEPING];
    }
    if (rounds == 0) {
      res.n_marked_first = n_conflicting;
      res.n_entries = E;
    }
    res.n_marked_left = n_conflicting;
    res.n_svertices = nseg;
    if (h_words[W_MARKED] == 0 || rounds == max_rounds)
      break;
    if (mode == 2 && h_words[W_S_SWEEPING] > 0)
      sw.sweep_rounds++;
    if (rounds >= N)
      return internal(ctx, 0x40000);  // (every round keeps a node: more rounds than nodes cannot be)
    // ---- repair ----
    BS_HIP(ctx, hipEventRecord(ev.e[4], st));
    uncross_spans_kernel<<<g, 256, 0, st>>>(segK, kscan, klist, mark, S.ring, S.noff, N, nr, segW, S.best[0], S.tie[0], S.forced, d_err);
    simplify_forced_round(st, N, segW, S.xy, S.cidx, S.c2, S.best[0], S.tie[0], S.forced, segK, S.best[1], S.tie[1],
                          d_words + W_CHANGED, d_err);
    BS_HIP(ctx, hipEventRecord(ev.e[5], st));
    repair_pending = true;  // (read after the next detection's first wait: no wait of its own)
    rounds++;
  }
  // ---- rings: the last detection ran over the final kept set: its scan and its marks hold ----
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  uncross_offsets_kernel<<<sweep((int64_t)nr + 1), 256, 0, st>>>(kscan, S.noff, nr, N, soff, area2, d_err);
  uncross_final_kernel<<<g, 256, 0, st>>>(segK, kscan, kept0, mark, mode ? sweep_marks(ctx) : nullptr, S.xy, S.z, S.right, S.ring,
                                          S.flag, S.noff, S.rot, N, nr, has_z, O, d_err);
  uncross_area_kernel<<<g, 256, 0, st>>>(O.xy, O.ring, soff, kscan, N, nr, area2, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  std::vector<int32_t> h_soff((size_t)nr + 1);
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_COUNT, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_soff.data(), soff, 4 * ((size_t)nr + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.s_ring_area2, area2, 8 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  if (h_words[W_ERR])
    return internal(ctx, h_words[W_ERR]);
  for (int32_t r = 0; r < nr; r++) {
    res.s_ring_offset[r] = h_soff[r];
    res.s_ring_vertices[r] = h_soff[r + 1] - h_soff[r];
    if (res.s_ring_vertices[r] < 2)
      return internal(ctx, 0x80000);
  }
  res.s_ring_offset[nr] = h_soff[nr];
  if (h_soff[0] != 0 || h_soff[nr] != res.n_svertices)
    return internal(ctx, 0x100000);
  res.n_forced = res.n_svertices - res.n_svertices_before;
  res.repair_rounds = rounds;
  res.max_cell_entries = h_words[W_MAXCELL];
  res.ms_detect = ms_detect;
  res.ms_repair = ms_repair;
  res.ms_rings = ev.ms(2, 3);
  return hand_over();
}

extern "C" int bs_clean_outlines_emit_dev(bs_ctx* ctx, int32_t* d_sxy, int32_t* d_sz, int32_t* d_right, uint8_t* d_flag)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!ctx->uc_valid)
    return fail(ctx, BS_ERR_INVALID, "clean outlines: emit without a successful count on this context");
  const int64_t nsv = ctx->uc_nsv;
  if ((nsv > 0 && (!d_sxy || !d_right || !d_flag)) || (nsv > 0 && ctx->uc_has_z && !d_sz) || (!ctx->uc_has_z && d_sz))
    return fail(ctx, BS_ERR_INVALID,
                "clean outlines: emit needs d_sxy, d_right and d_flag, and d_sz exactly when the count had a top image");
  ctx->uc_ms_emit = 0;
  if (nsv == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events<2> ev;
  BS_HIP(ctx, hipEventCreate(&ev.e[0]));
  BS_HIP(ctx, hipEventCreate(&ev.e[1]));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  uncross_emit_kernel<<<sweep(nsv), 256, 0, st>>>(final_arrays(ctx->uc), nsv, reinterpret_cast<int2*>(d_sxy), d_sz, d_right, d_flag);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  ctx->uc_ms_emit = ev.ms(0, 1);
  return BS_OK;
}

extern "C" int bs_clean_outlines(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height,
                                 int32_t n_labels, int64_t num, int64_t den, int32_t max_rounds, int32_t cell_log2,
                                 struct bs_clean_outlines* out, struct bs_simple_outlines* simple, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->uc_valid = false;
  if (!label || !out || bad_image(width, height))
    return fail(ctx, BS_ERR_INVALID, "clean outlines: null pointer, width or height < 1 or width * height >= 2^29");
  const size_t npix = (size_t)width * height;
  DevBuf* B = ctx->uc;
  Staging S(ctx);
  const int32_t* d_label = S.upload(B[UC_IN_LABEL], label, npix);
  const int32_t* d_top = S.upload(B[UC_IN_TOP], top, 4 * npix);
  if (!S.ok())
    return S.status();
  Chain ch;  // (its clean outlines are this call's own result)
  int rc = bs_clean_outlines_count_dev(ctx, d_label, d_top, width, height, n_labels, num, den, max_rounds, cell_log2, &ch.clean,
                                       &ch.simple, &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_plain = ch.has_simple = ch.has_clean = true;
  rc = kept_vertices_to_host(ctx, S, ch.clean, {B[UC_OUT_XY], B[UC_OUT_Z], B[UC_OUT_RIGHT], B[UC_OUT_FLAG]},
                             bs_clean_outlines_emit_dev, &ctx->uc_ms_emit, "clean outlines: host allocation");
  if (rc != BS_OK)
    return rc;
  ch.hand_over(nullptr, out, simple, plain);
  return BS_OK;
}

// The simplified writer's format with a first line of its own (include/bs_api.h).
extern "C" int bs_clean_outlines_write_obj(const struct bs_clean_outlines* o, int32_t bin, const int32_t* origin, const char* path)
{
  if (!o || !path || bin < 1 || o->n_rings < 0 || o->n_svertices < 0 || o->n_labels < 0)
    return BS_ERR_INVALID;
  if (!o->s_ring_offset || !o->label_ring_offset || (o->n_rings > 0 && (!o->ring_label || !o->ring_area2)) ||
      (o->n_svertices > 0 && !o->sxy))
    return BS_ERR_INVALID;
  if (o->s_ring_offset[0] != 0 || o->s_ring_offset[o->n_rings] != o->n_svertices)
    return BS_ERR_INVALID;
  for (int64_t r = 0; r < o->n_rings; r++) {
    const int32_t l = o->ring_label[r];
    if (o->s_ring_offset[r + 1] < o->s_ring_offset[r] || l < 0 || l >= o->n_labels || o->label_ring_offset[l] > r)
      return BS_ERR_INVALID;
  }
  FILE* fo = fopen(path, "w");
  if (!fo)
    return BS_ERR_INVALID;
  fprintf(fo, "# clean outlines: %d labels, %lld rings, %lld vertices, tol2 %d/%d, repair_rounds %lld, n_forced %lld\n", o->n_labels,
          (long long)o->n_rings, (long long)o->n_svertices, o->tol_num, o->tol_den, (long long)o->repair_rounds,
          (long long)o->n_forced);
  return write_kept_rings(fo, o, bin, origin);
}
