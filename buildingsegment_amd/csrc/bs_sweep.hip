// bs_sweep.hip -- the sweep detection of the clean outlines (DESIGN.md "Sweeps"; the definition is written down in
// include/bs_api.h under "clean outlines", paragraph "sweeps"): the segments whose lens -- the dropped path closed by the
// chord -- winds around a kept vertex that does not lie on it.
//   bitmap   a bit per lattice corner, set at every kept node
//   runs     a thread per node: its segment from the kept scan and list, the ray axis by the chord's dominant direction (the
//            coordinates are swapped where |dx| < |dy|, so that the rays below are always vertical), and the lattice lines
//            that the run to the next node crosses, half-open: one item per line; an exclusive sum
//   items    a thread per item (bisection of the sum): the corners of its line between the run and the chord's crossing of
//            that line -- or the nearer chord end where the chord does not cross it; an exclusive sum of the corner counts
//   test     a thread per candidate corner (bisection of the sum): a corner that is a kept vertex and neither end of the
//            segment is a hit, and the hit is tested exactly at once -- by its thread where the path has at most
//            SWEEP_WAVE_CAP runs, else by the whole wave striding the runs -- boundary, signed crossings of the upward ray,
//            and the first item of that line that holds the corner, so that a (corner, segment) pair is counted once
//   marks    sweeping and sweeping-only segments counted, the marks OR-ed into the conflict marks in mode 2
// On a line the signed crossings of a closed polygon sum to zero, so the winding around w is the sum over the runs on w's
// line of +-[w between the run and the reference]: a corner outside every item's interval has winding 0.  No thread walks a
// ring in the broad phase; an item's time does not depend on its interval.  Every index read from memory is checked before
// it is used as an address.  Marks are plain stores of 1; sums of different lenses never meet in one counter.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>

#include "bs_host.h"
#include "bs_sweep.h"

namespace bs {
namespace {

constexpr int32_t KEPT = -1;     // seg.x of a kept node (bs_simplify.hip)
constexpr int E_RUNS = 1024, E_ITEMS = 2048, E_TEST = 4096;  // phase bits of the error word

struct SweepDev {
  const int2* segK;
  const int32_t *kscan, *klist;
  const int2* xy;
  const int32_t *ring, *noff;
  int32_t N, nr, width, height;
};

struct Lens {  // the segment that holds a node
  int32_t j, L, R, r0, r1;
  int2 a, b;  // the chord's ends, swapped coordinates where T
  bool T, lens;
};

struct ItemCount {  // the item count of node q, 0 behind the last
  const int32_t* cnt;
  int32_t N;
  __host__ __device__ long long operator()(int32_t q) const { return q < N ? cnt[q] : 0; }
};

__device__ inline int2 tr(int2 p, bool T) { return T ? make_int2(p.y, p.x) : p; }
__device__ inline int32_t next_of(int32_t q, int32_t r0, int32_t r1) { return q + 1 < r1 ? q + 1 : r0; }
__device__ inline bool in_image(const SweepDev& D, int2 p)
{
  return (uint32_t)p.x <= (uint32_t)D.width && (uint32_t)p.y <= (uint32_t)D.height;
}

__device__ inline bool load_lens(const SweepDev& D, int32_t q, Lens& s)
{
  const int32_t r = D.ring[q];
  if ((uint32_t)r >= (uint32_t)D.nr)
    return false;
  s.r0 = D.noff[r];
  s.r1 = D.noff[r + 1];
  if (s.r0 < 0 || s.r0 > q || s.r1 <= q || s.r1 > D.N)
    return false;
  const int32_t nseg = D.kscan[D.N], k = D.kscan[q];
  s.j = D.segK[q].x == KEPT ? k : k - 1;
  if (nseg > D.N || (uint32_t)s.j >= (uint32_t)nseg)
    return false;
  s.L = D.klist[s.j];
  if (s.L < s.r0 || s.L > q)
    return false;
  const int32_t kend = D.kscan[s.r1];
  if (kend <= s.j || kend > nseg)
    return false;
  s.R = s.j + 1 < kend ? D.klist[s.j + 1] : s.r0;
  if (s.R < s.r0 || s.R >= s.r1)
    return false;
  s.lens = s.R != s.L && next_of(s.L, s.r0, s.r1) != s.R;
  const int2 a = D.xy[s.L], b = D.xy[s.R];
  if (!in_image(D, a) || !in_image(D, b))
    return false;
  s.T = abs(b.x - a.x) < abs(b.y - a.y);
  s.a = tr(a, s.T);
  s.b = tr(b, s.T);
  return true;
}

// the chord's crossing of the line X as floor and ceiling of its Y, or the Y of the nearer end where it does not cross
__device__ inline void chord_ref(int2 a, int2 b, int X, int& flo, int& cei)
{
  const int mn = min(a.x, b.x), mx = max(a.x, b.x);
  if (X >= mn && X < mx) {
    long long dx = b.x - a.x, num = (long long)(X - a.x) * (b.y - a.y);
    if (dx < 0)
      dx = -dx, num = -num;
    long long f = num / dx;
    const bool frac = num % dx != 0;
    if (frac && num < 0)
      f--;
    flo = a.y + (int)f;
    cei = flo + (frac ? 1 : 0);
  } else {
    const int2 e = ((X < mn) == (a.x <= b.x)) ? a : b;
    flo = cei = e.y;
  }
}

__device__ inline long long orient(int2 a, int2 b, int2 p)
{
  return (long long)(b.x - a.x) * (p.y - a.y) - (long long)(b.y - a.y) * (p.x - a.x);
}

__device__ inline int wave_sum(int v)
{
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_xor(v, o);
  return v;
}

// ---- bitmap ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sweep_bitmap_kernel(SweepDev D, uint32_t* __restrict__ bits, int* __restrict__ err)
{
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < D.N; q += (int64_t)gridDim.x * blockDim.x) {
    if (D.segK[q].x != KEPT)
      continue;
    const int2 p = D.xy[q];
    if (!in_image(D, p)) {
      atomicOr(err, E_RUNS);
      continue;
    }
    const uint32_t c = (uint32_t)p.y * (uint32_t)(D.width + 1) + (uint32_t)p.x;
    atomicOr(bits + (c >> 5), 1u << (c & 31));
  }
}

// ---- runs ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sweep_runs_kernel(SweepDev D, int32_t* __restrict__ icnt, int* __restrict__ words)
{
  __shared__ int s_acc[2];  // the lens segments and the swapped items of the workgroup: one atomic each to memory
  if (threadIdx.x < 2)
    s_acc[threadIdx.x] = 0;
  __syncthreads();
  int32_t lens = 0, ct = 0;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < D.N; q += (int64_t)gridDim.x * blockDim.x) {
    int32_t c = 0;
    Lens s;
    if (!load_lens(D, (int32_t)q, s)) {
      atomicOr(words + W_ERR, E_RUNS);
    } else if (s.lens) {
      lens += q == s.L;
      const int2 pr = D.xy[q], nr_ = D.xy[next_of((int32_t)q, s.r0, s.r1)];
      if (!in_image(D, pr) || !in_image(D, nr_) || (pr.x != nr_.x && pr.y != nr_.y)) {
        atomicOr(words + W_ERR, E_RUNS);  // (a run between adjacent nodes is axis-parallel)
      } else {
        const int2 p = tr(pr, s.T), n = tr(nr_, s.T);
        if (p.y == n.y)
          c = abs(n.x - p.x);
        ct += s.T ? c : 0;
      }
    }
    icnt[q] = c;
  }
  lens = wave_sum(lens);
  ct = wave_sum(ct);
  if ((threadIdx.x & 63) == 0) {
    if (lens > 0)
      atomicAdd(&s_acc[0], lens);
    if (ct > 0)
      atomicAdd(&s_acc[1], ct);
  }
  __syncthreads();
  if (threadIdx.x == 0 && s_acc[0] > 0)
    atomicAdd(words + W_S_LENS, s_acc[0]);
  if (threadIdx.x == 0 && s_acc[1] > 0)
    atomicAdd(words + W_S_ITEMS_T, s_acc[1]);
}

// ---- items -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sweep_items_kernel(SweepDev D, const int32_t* __restrict__ icnt,
                                                          const long long* __restrict__ ioff, int32_t n_items,
                                                          int4* __restrict__ item, int32_t* __restrict__ ccnt, int* __restrict__ err)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_items; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t lo = 0, hi = D.N;  // ioff[lo] <= i < ioff[hi]: the last node whose items start at or in front of i
    while (hi - lo > 1) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      if (ioff[mid] <= i)
        lo = mid;
      else
        hi = mid;
    }
    const int32_t q = lo;
    const long long l = i - ioff[q];
    int4 it = make_int4(0, 0, 0, -1);
    Lens s;
    if (l < 0 || l >= icnt[q] || !load_lens(D, q, s) || !s.lens) {
      atomicOr(err, E_ITEMS);
    } else {
      const int2 p = tr(D.xy[q], s.T), n = tr(D.xy[next_of(q, s.r0, s.r1)], s.T);
      const int X = min(p.x, n.x) + (int)l;
      int flo, cei;
      chord_ref(s.a, s.b, X, flo, cei);
      it = make_int4((int)((uint32_t)q | (s.T ? 0x80000000u : 0u)), X, min(p.y, flo), max(p.y, cei));
    }
    item[i] = it;
    ccnt[i] = it.w - it.z + 1;
  }
}

struct CornerCount {  // the corner count of item i, 0 behind the last
  const int32_t* cnt;
  int32_t n;
  __host__ __device__ long long operator()(int32_t i) const { return i < n ? cnt[i] : 0; }
};

// ---- test ------------------------------------------------------------------------------------------------------------------
struct Exact {
  int wn;         // signed crossings of the path's runs with the upward ray
  int32_t first;  // the first run of w's line whose interval holds w
  bool onb;       // w on a run
};

// the runs start, start + stride, ... of the path against w
__device__ inline Exact exact_runs(const SweepDev& D, const Lens& s, int2 w, int flo, int cei, int32_t start, int32_t stride,
                                   int32_t cnt, bool& bad)
{
  Exact x{0, INT_MAX, false};
  const int32_t nn = s.r1 - s.r0;
  for (int32_t e = start; e < cnt; e += stride) {
    int32_t qi = s.L + e;
    if (qi >= s.r1)
      qi -= nn;
    if (qi < s.r0 || qi >= s.r1) {
      bad = true;
      break;
    }
    const int2 p = tr(D.xy[qi], s.T), n = tr(D.xy[next_of(qi, s.r0, s.r1)], s.T);
    if (p.x == n.x) {
      if (w.x == p.x && w.y >= min(p.y, n.y) && w.y <= max(p.y, n.y))
        x.onb = true;
    } else if (p.y == n.y) {
      const int mn = min(p.x, n.x), mx = max(p.x, n.x);
      if (w.y == p.y && w.x >= mn && w.x <= mx)
        x.onb = true;
      if (w.x >= mn && w.x < mx) {
        if (p.y > w.y)
          x.wn += p.x < n.x ? 1 : -1;
        if (w.y >= min(p.y, flo) && w.y <= max(p.y, cei))
          x.first = min(x.first, e);
      }
    } else {
      bad = true;
    }
  }
  return x;
}

// the chord's share, and what one exact test leaves: the mark, the counts
__device__ inline void exact_end(const Lens& s, int2 w, Exact x, int32_t ecur, bool wave, uint8_t* __restrict__ smark,
                                 int* __restrict__ words)
{
  const int2 a = s.a, b = s.b;
  const long long o = orient(b, a, w);  // the chord runs b -> a
  if (o == 0 && w.x >= min(a.x, b.x) && w.x <= max(a.x, b.x) && w.y >= min(a.y, b.y) && w.y <= max(a.y, b.y))
    x.onb = true;
  if (w.x >= min(a.x, b.x) && w.x < max(a.x, b.x)) {
    if (b.x < a.x && o < 0)
      x.wn += 1;
    else if (b.x > a.x && o > 0)
      x.wn -= 1;
  }
  atomicAdd(words + W_S_EXACT, 1);
  if (wave)
    atomicAdd(words + W_S_WAVE, 1);
  if (x.onb || x.wn == 0) {
    atomicAdd(words + W_S_REJECT, 1);
    return;
  }
  smark[s.j] = SM_SWEEPING;
  atomicMax(words + W_S_MAXW, abs(x.wn));
  if (x.first == ecur)
    atomicAdd(words + W_S_PAIRS, 1);
}

__global__ __launch_bounds__(256) void sweep_test_kernel(SweepDev D, const long long* __restrict__ coff, const int4* __restrict__ item,
                                                         int32_t n_items, const uint32_t* __restrict__ bits,
                                                         uint8_t* __restrict__ smark, int* __restrict__ words)
{
  const int lane = threadIdx.x & 63;
  const long long total = coff[n_items];
  if (total < 0) {
    atomicOr(words + W_ERR, E_TEST);
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    words[W_S_CAND_LO] = (int)(uint32_t)(total & 0xffffffffll);
    words[W_S_CAND_HI] = (int)(total >> 32);
  }
  const long long n64 = (total + 63) & ~63ll;
  for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < n64; c += (long long)gridDim.x * blockDim.x) {
    bool hit = false;
    Lens s{};
    int2 w = make_int2(0, 0);
    int32_t q = 0, ecur = 0, cnt = 0;
    if (c < total) {
      int32_t lo = 0, hi = n_items;  // coff[lo] <= c < coff[hi]
      while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (coff[mid] <= c)
          lo = mid;
        else
          hi = mid;
      }
      const int4 it = item[lo];
      const bool T = it.x < 0;
      q = it.x & 0x7fffffff;
      const long long y = it.z + (c - coff[lo]);
      w = make_int2(it.y, (int)y);
      const int2 real = tr(w, T);
      if (q >= D.N || y < it.z || y > it.w || !in_image(D, real)) {
        atomicOr(words + W_ERR, E_TEST);
      } else {
        const uint32_t ci = (uint32_t)real.y * (uint32_t)(D.width + 1) + (uint32_t)real.x;
        if ((bits[ci >> 5] >> (ci & 31)) & 1u) {
          if (!load_lens(D, q, s) || !s.lens || s.T != T) {
            atomicOr(words + W_ERR, E_TEST);
          } else if (!(w.x == s.a.x && w.y == s.a.y) && !(w.x == s.b.x && w.y == s.b.y)) {
            const int32_t nn = s.r1 - s.r0;
            hit = true;
            cnt = s.R - s.L;
            if (cnt <= 0)
              cnt += nn;
            ecur = q - s.L;
          }
        }
      }
    }
    bool bad = false;
    if (hit && cnt <= SWEEP_WAVE_CAP) {
      int flo, cei;
      chord_ref(s.a, s.b, w.x, flo, cei);
      const Exact x = exact_runs(D, s, w, flo, cei, 0, 1, cnt, bad);
      if (!bad)
        exact_end(s, w, x, ecur, false, smark, words);
    }
    unsigned long long longs = __ballot(hit && cnt > SWEEP_WAVE_CAP);
    while (longs) {  // (the same in every lane of the wave)
      const int src = __ffsll((long long)longs) - 1;
      longs &= longs - 1;
      const int32_t wq = __shfl(q, src), we = __shfl(ecur, src), wc = __shfl(cnt, src);
      const int2 ww = make_int2(__shfl(w.x, src), __shfl(w.y, src));
      Lens ws;
      if (!load_lens(D, wq, ws)) {
        bad = true;
        continue;
      }
      int flo, cei;
      chord_ref(ws.a, ws.b, ww.x, flo, cei);
      Exact x = exact_runs(D, ws, ww, flo, cei, lane, 64, wc, bad);
      x.wn = wave_sum(x.wn);
      x.onb = __any(x.onb);
      for (int o = 32; o > 0; o >>= 1)
        x.first = min(x.first, __shfl_xor(x.first, o));
      const bool any_bad = __any(bad);
      if (lane == 0 && !any_bad)
        exact_end(ws, ww, x, we, true, smark, words);
    }
    if (bad)
      atomicOr(words + W_ERR, E_TEST);
  }
}

// ---- marks -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sweep_marks_kernel(uint8_t* __restrict__ smark, uint8_t* __restrict__ mark, int32_t nseg,
                                                          int mode, int* __restrict__ words)
{
  const int lane = threadIdx.x & 63;
  const int64_t n64 = ((int64_t)nseg + 63) & ~(int64_t)63;
  for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n64; j += (int64_t)gridDim.x * blockDim.x) {
    int s = 0, only = 0;
    if (j < nseg && smark[j]) {
      s = 1;
      only = mark[j] == 0;
      smark[j] = (uint8_t)(SM_SWEEPING | (only ? SM_ONLY : 0));
      if (mode == 2)
        mark[j] = 1;
    }
    s = wave_sum(s);
    only = wave_sum(only);
    if (lane == 0 && s > 0) {
      atomicAdd(words + W_S_SWEEPING, s);
      if (only > 0)
        atomicAdd(words + W_S_ONLY, only);
    }
  }
}

SweepDev dev_of(const SweepRun& R) { return SweepDev{R.segK, R.kscan, R.klist, R.xy, R.ring, R.noff, R.N, R.nr, R.width, R.height}; }

}  // namespace

int sweep_begin(bs_ctx* ctx, const SweepRun& R, long long* h_items)
{
  DevBuf* B = ctx->sw;
  const size_t words = ((size_t)(R.width + 1) * (size_t)(R.height + 1) + 31) / 32;
  BS_HIP(ctx, B[SW_BITS].reserve(4 * words));
  BS_HIP(ctx, B[SW_SMARK].reserve((size_t)R.N));
  BS_HIP(ctx, B[SW_ICNT].reserve(4 * (size_t)R.N));
  BS_HIP(ctx, B[SW_IOFF].reserve(8 * ((size_t)R.N + 1)));
  int32_t* icnt = B[SW_ICNT].as<int32_t>();
  long long* ioff = B[SW_IOFF].as<long long>();
  hipcub::CountingInputIterator<int32_t> idx(0);
  hipcub::TransformInputIterator<long long, ItemCount, hipcub::CountingInputIterator<int32_t>> ic(idx, ItemCount{icnt, R.N});
  auto scan = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, ic, ioff, R.N + 1, R.st); };
  BS_HIP(ctx, cub_room(B[SW_TMP], scan));
  const SweepDev D = dev_of(R);
  BS_HIP(ctx, hipMemsetAsync(R.d_words + W_S_LENS, 0, 4 * (W_COUNT - W_S_LENS), R.st));
  BS_HIP(ctx, hipMemsetAsync(B[SW_BITS].p, 0, 4 * words, R.st));
  sweep_bitmap_kernel<<<sweep(R.N), 256, 0, R.st>>>(D, B[SW_BITS].as<uint32_t>(), R.d_words + W_ERR);
  sweep_runs_kernel<<<sweep(R.N), 256, 0, R.st>>>(D, icnt, R.d_words);
  BS_HIP(ctx, cub_run(B[SW_TMP], scan));
  BS_HIP(ctx, hipMemcpyAsync(h_items, ioff + R.N, 8, hipMemcpyDeviceToHost, R.st));
  return BS_OK;
}

int sweep_detect(bs_ctx* ctx, const SweepRun& R, int32_t nseg, long long n_items, uint8_t* mark)
{
  DevBuf* B = ctx->sw;
  uint8_t* smark = B[SW_SMARK].as<uint8_t>();
  BS_HIP(ctx, hipMemsetAsync(smark, 0, (size_t)nseg, R.st));
  if (n_items > 0) {
    const int32_t n = (int32_t)n_items;
    BS_HIP(ctx, B[SW_ITEM].reserve(16 * (size_t)n));
    BS_HIP(ctx, B[SW_CCNT].reserve(4 * (size_t)n));
    BS_HIP(ctx, B[SW_COFF].reserve(8 * ((size_t)n + 1)));
    int4* item = B[SW_ITEM].as<int4>();
    int32_t* ccnt = B[SW_CCNT].as<int32_t>();
    long long* coff = B[SW_COFF].as<long long>();
    hipcub::CountingInputIterator<int32_t> idx(0);
    hipcub::TransformInputIterator<long long, CornerCount, hipcub::CountingInputIterator<int32_t>> cc(idx, CornerCount{ccnt, n});
    auto scan = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, cc, coff, n + 1, R.st); };
    BS_HIP(ctx, cub_room(B[SW_TMP], scan));
    const SweepDev D = dev_of(R);
    sweep_items_kernel<<<sweep(n), 256, 0, R.st>>>(D, B[SW_ICNT].as<int32_t>(), B[SW_IOFF].as<long long>(), n, item, ccnt,
                                                   R.d_words + W_ERR);
    BS_HIP(ctx, cub_run(B[SW_TMP], scan));
    sweep_test_kernel<<<SWEEP_CAP, 256, 0, R.st>>>(D, coff, item, n, B[SW_BITS].as<uint32_t>(), smark, R.d_words);
  }
  sweep_marks_kernel<<<sweep(nseg), 256, 0, R.st>>>(smark, mark, nseg, R.mode, R.d_words);
  return BS_OK;
}

}  // namespace bs
