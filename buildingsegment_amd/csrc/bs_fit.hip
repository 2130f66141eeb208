// bs_fit.hip -- every plane's exact centroid, least-squares normal and residuals from the points that carry its label
// ("Plane fit"; the definition is written down in include/bs_api.h).
//   A. sums       one pass over the points: count, coordinate sums and box per plane; the domain check of every point
//      verdict    one thread per plane: centroid, status, dev_sum (the remainder of the centroid's division)
//   B. moments    one pass: the six second moments about the centroid, fitted planes only
//      solve      one thread per plane: covariance and smallest eigenvector (bs_normal.h, the tail of stage 2)
//   C. residuals  one pass: the truncated distance of every point to its plane, and max |r|, sum |r|, sum r^2 per plane
// The three passes reduce by label the same way: a wave whose labelled lanes all carry one plane reduces in registers
// and adds once; otherwise every lane adds for itself; planes 1 .. FIT_CAP are added in LDS tables that a workgroup
// flushes once, the rest with global atomics.  One workgroup of 1024 threads per CU owns (almost) the whole LDS: the
// tables then hold every plane of a tile of some thousand planes, whatever the order of the points.
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_common.h"
#include "bs_host.h"
#include "bs_normal.h"

namespace bs {
namespace {

constexpr int FIT_CAP = 3072;      // planes 1 .. FIT_CAP: reduced in LDS (156 KB in pass A, 144 KB in B, 60 KB in C)
constexpr int FIT_THREADS = 1024;  // one workgroup per CU
constexpr int FIT_ITEMS = 4;       // points per thread and trip: a workgroup takes 4096 consecutive points
constexpr int FIT_GRID = 256;      // workgroups of a point pass at most (then they stride over the cloud)
constexpr int32_t FIT_LIM = 1 << 23;
// scratch of bs_ctx::ft
enum { FT_TAB, FT_MISC, FT_IN_XYZ, FT_IN_PLANE, FT_OUT };

struct Fit {  // per plane, device: entry p - 1 is plane p
  unsigned long long* cnt;   // [m]
  unsigned long long* sum;   // [m][3]  (two's complement)
  unsigned long long* mom;   // [m][6]
  unsigned long long* rsum;  // [m]
  unsigned long long* rsq;   // [m]
  long long* dev;            // [m][3]
  double* normal;            // [m][3]
  int4* cen;                 // [m] centre x, y, z and the status
  int32_t* box;              // [m][6]
  int32_t* rmax;             // [m]
};
constexpr size_t FIT_BYTES = 8 * 18 + 16 + 4 * 7;  // per plane

__global__ __launch_bounds__(256) void fit_init_kernel(Fit f, int32_t m, int* bad)
{
  const int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0)
    *bad = 0;
  if (c >= m)
    return;
  f.cnt[c] = f.rsum[c] = f.rsq[c] = 0;
  for (int a = 0; a < 3; a++) {
    f.sum[3 * c + a] = 0;
    f.box[6 * c + a] = INT32_MAX;
    f.box[6 * c + 3 + a] = INT32_MIN;
  }
  for (int a = 0; a < 6; a++)
    f.mom[6 * c + a] = 0;
  f.rmax[c] = 0;
}

__device__ inline unsigned long long wave_sum(unsigned long long v)
{
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_xor(v, o);
  return v;
}
__device__ inline int32_t wave_min(int32_t v)
{
  for (int o = 32; o > 0; o >>= 1)
    v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ inline int32_t wave_max(int32_t v)
{
  for (int o = 32; o > 0; o >>= 1)
    v = max(v, __shfl_xor(v, o));
  return v;
}

// Do the labelled lanes (s >= 0; at least one) of the wave all carry one plane?  *s0 = the first labelled lane's.
__device__ inline bool wave_one_label(int32_t s, unsigned long long labelled, int32_t* s0)
{
  *s0 = __shfl(s, __ffsll((long long)labelled) - 1);
  return __ballot(s >= 0 && s != *s0) == 0;
}

struct Pts {  // the FIT_ITEMS points of a thread in one trip: s = plane - 1, or -1 (no point, or a label that is ignored)
  int32_t x[FIT_ITEMS], y[FIT_ITEMS], z[FIT_ITEMS], s[FIT_ITEMS];
};

__device__ inline void load_points(const int32_t* __restrict__ xyz, int64_t n, const int32_t* __restrict__ plane,
                                   int32_t npl, int64_t base, Pts& p)
{
#pragma unroll
  for (int j = 0; j < FIT_ITEMS; j++) {
    const int64_t i = base + j * FIT_THREADS + threadIdx.x;
    p.x[j] = p.y[j] = p.z[j] = 0;
    p.s[j] = -1;
    if (i < n) {
      p.x[j] = xyz[3 * i];
      p.y[j] = xyz[3 * i + 1];
      p.z[j] = xyz[3 * i + 2];
      const int32_t l = plane[i];
      p.s[j] = (l >= 1 && l <= npl) ? l - 1 : -1;
    }
  }
}

// ---- pass A ------------------------------------------------------------------------------------------------------
__device__ inline void sums_global(const Fit& f, int32_t s, unsigned cnt, const long long* v, const int32_t* lo,
                                   const int32_t* hi)
{
  atomicAdd(f.cnt + s, (unsigned long long)cnt);
  for (int a = 0; a < 3; a++) {
    atomicAdd(f.sum + 3 * s + a, (unsigned long long)v[a]);
    atomicMin(f.box + 6 * s + a, lo[a]);
    atomicMax(f.box + 6 * s + 3 + a, hi[a]);
  }
}

__global__ __launch_bounds__(FIT_THREADS) void sums_kernel(const int32_t* __restrict__ xyz, int64_t n,
                                                           const int32_t* __restrict__ plane, int32_t npl, Fit f,
                                                           int* __restrict__ bad)
{
  __shared__ unsigned s_cnt[FIT_CAP];
  __shared__ unsigned long long s_sum[3 * FIT_CAP];
  __shared__ int32_t s_lo[3 * FIT_CAP], s_hi[3 * FIT_CAP];
  const int cap = min(npl, FIT_CAP);
  for (int k = threadIdx.x; k < cap; k += FIT_THREADS) {
    s_cnt[k] = 0;
    for (int a = 0; a < 3; a++) {
      s_sum[3 * k + a] = 0;
      s_lo[3 * k + a] = INT32_MAX;
      s_hi[3 * k + a] = INT32_MIN;
    }
  }
  __syncthreads();
  const int64_t tile = (int64_t)FIT_THREADS * FIT_ITEMS;
  for (int64_t base = blockIdx.x * tile; base < n; base += gridDim.x * tile) {  // (whole waves stay together)
    Pts p;
    load_points(xyz, n, plane, npl, base, p);
#pragma unroll
    for (int j = 0; j < FIT_ITEMS; j++) {
      const int32_t c[3] = {p.x[j], p.y[j], p.z[j]};
      if (c[0] <= -FIT_LIM || c[0] >= FIT_LIM || c[1] <= -FIT_LIM || c[1] >= FIT_LIM || c[2] <= -FIT_LIM || c[2] >= FIT_LIM)
        atomicOr(bad, 1);  // (of any point, labelled or not)
      const int32_t s = p.s[j];
      const unsigned long long labelled = __ballot(s >= 0);
      if (!labelled)
        continue;
      int32_t s0;
      if (wave_one_label(s, labelled, &s0)) {  // one plane in the wave (clouds in spatial order): reduce in registers
        long long v[3];
        int32_t lo[3], hi[3];
        for (int a = 0; a < 3; a++) {
          v[a] = (long long)wave_sum(s >= 0 ? (unsigned long long)(long long)c[a] : 0ull);
          lo[a] = wave_min(s >= 0 ? c[a] : INT32_MAX);
          hi[a] = wave_max(s >= 0 ? c[a] : INT32_MIN);
        }
        if ((threadIdx.x & 63) == 0) {
          const unsigned cnt = (unsigned)__popcll(labelled);
          if (s0 < FIT_CAP) {
            atomicAdd(s_cnt + s0, cnt);
            for (int a = 0; a < 3; a++) {
              atomicAdd(s_sum + 3 * s0 + a, (unsigned long long)v[a]);
              atomicMin(s_lo + 3 * s0 + a, lo[a]);
              atomicMax(s_hi + 3 * s0 + a, hi[a]);
            }
          } else {
            sums_global(f, s0, cnt, v, lo, hi);
          }
        }
      } else if (s >= 0) {
        if (s < FIT_CAP) {
          atomicAdd(s_cnt + s, 1u);
          for (int a = 0; a < 3; a++) {
            atomicAdd(s_sum + 3 * s + a, (unsigned long long)(long long)c[a]);
            atomicMin(s_lo + 3 * s + a, c[a]);
            atomicMax(s_hi + 3 * s + a, c[a]);
          }
        } else {
          const long long v[3] = {c[0], c[1], c[2]};
          sums_global(f, s, 1u, v, c, c);
        }
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < cap; k += FIT_THREADS)
    if (s_cnt[k]) {
      const long long v[3] = {(long long)s_sum[3 * k], (long long)s_sum[3 * k + 1], (long long)s_sum[3 * k + 2]};
      sums_global(f, k, s_cnt[k], v, s_lo + 3 * k, s_hi + 3 * k);
    }
}

// centroid, verdict and dev_sum of every plane
__global__ __launch_bounds__(256) void verdict_kernel(Fit f, int32_t npl)
{
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npl)
    return;
  const long long n = (long long)f.cnt[p];
  long long c[3] = {0, 0, 0}, D = 0;
  int32_t st = 1;
  if (n > 0) {
    for (int a = 0; a < 3; a++) {
      c[a] = (long long)f.sum[3 * p + a] / n;  // truncated towards zero
      D = max(D, max((long long)f.box[6 * p + 3 + a] - c[a], c[a] - (long long)f.box[6 * p + a]));
    }
    if (n >= 3) {
      // 3 n D^2 >= 2^63  <=>  D^2 >= ceil(2^63 / 3n): D < 2^25 and 3n < 2^31, so both sides fit 64 bits
      const unsigned long long t = 3ull * (unsigned long long)n, need = ((1ull << 63) + t - 1) / t;
      st = (unsigned long long)D * (unsigned long long)D >= need ? 2 : 0;
    }
  }
  for (int a = 0; a < 3; a++)
    f.dev[3 * p + a] = st == 0 ? (long long)f.sum[3 * p + a] - n * c[a] : 0;
  f.cen[p] = make_int4((int32_t)c[0], (int32_t)c[1], (int32_t)c[2], st);
}

// ---- pass B ------------------------------------------------------------------------------------------------------
__device__ inline void moments_global(const Fit& f, int32_t s, const unsigned long long* q)
{
  for (int a = 0; a < 6; a++)
    if (q[a])
      atomicAdd(f.mom + 6 * s + a, q[a]);
}

__global__ __launch_bounds__(FIT_THREADS) void moments_kernel(const int32_t* __restrict__ xyz, int64_t n,
                                                              const int32_t* __restrict__ plane, int32_t npl, Fit f)
{
  __shared__ unsigned long long s_mom[6 * FIT_CAP];
  const int cap = min(npl, FIT_CAP);
  for (int k = threadIdx.x; k < 6 * cap; k += FIT_THREADS)
    s_mom[k] = 0;
  __syncthreads();
  const int64_t tile = (int64_t)FIT_THREADS * FIT_ITEMS;
  for (int64_t base = blockIdx.x * tile; base < n; base += gridDim.x * tile) {
    Pts p;
    load_points(xyz, n, plane, npl, base, p);
#pragma unroll
    for (int j = 0; j < FIT_ITEMS; j++) {
      int32_t s = p.s[j];
      unsigned long long q[6] = {0, 0, 0, 0, 0, 0};
      if (s >= 0) {
        const int4 c = f.cen[s];
        if (c.w != 0) {
          s = -1;  // not fitted
        } else {
          const long long dx = p.x[j] - c.x, dy = p.y[j] - c.y, dz = p.z[j] - c.z;
          q[0] = (unsigned long long)(dx * dx);
          q[1] = (unsigned long long)(dx * dy);
          q[2] = (unsigned long long)(dx * dz);
          q[3] = (unsigned long long)(dy * dy);
          q[4] = (unsigned long long)(dy * dz);
          q[5] = (unsigned long long)(dz * dz);
        }
      }
      const unsigned long long labelled = __ballot(s >= 0);
      if (!labelled)
        continue;
      int32_t s0;
      if (wave_one_label(s, labelled, &s0)) {
        for (int a = 0; a < 6; a++)
          q[a] = wave_sum(q[a]);  // (the other lanes hold zeros)
        if ((threadIdx.x & 63) == 0) {
          if (s0 < FIT_CAP) {
            for (int a = 0; a < 6; a++)
              atomicAdd(s_mom + 6 * s0 + a, q[a]);
          } else {
            moments_global(f, s0, q);
          }
        }
      } else if (s >= 0) {
        if (s < FIT_CAP) {
          for (int a = 0; a < 6; a++)
            atomicAdd(s_mom + 6 * s + a, q[a]);
        } else {
          moments_global(f, s, q);
        }
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < cap; k += FIT_THREADS)
    moments_global(f, k, s_mom + 6 * k);
}

// covariance and normal of every plane
__global__ __launch_bounds__(256) void solve_kernel(Fit f, int32_t npl)
{
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npl)
    return;
  V3 nv = {0, 0, 1};
  if (f.cen[p].w == 0) {
    const double dn = (double)(long long)f.cnt[p];
    const double e0 = (double)f.dev[3 * p] / dn, e1 = (double)f.dev[3 * p + 1] / dn, e2 = (double)f.dev[3 * p + 2] / dn;
    const long long* m = reinterpret_cast<const long long*>(f.mom + 6 * p);
    Sym3 C;
    C.a00 = (double)m[0] / dn - e0 * e0;
    C.a01 = (double)m[1] / dn - e0 * e1;
    C.a02 = (double)m[2] / dn - e0 * e2;
    C.a11 = (double)m[3] / dn - e1 * e1;
    C.a12 = (double)m[4] / dn - e1 * e2;
    C.a22 = (double)m[5] / dn - e2 * e2;
    nv = normal_from_covariance(C);
  }
  f.normal[3 * p] = nv.x;
  f.normal[3 * p + 1] = nv.y;
  f.normal[3 * p + 2] = nv.z;
}

// ---- pass C ------------------------------------------------------------------------------------------------------
__device__ inline void residuals_global(const Fit& f, int32_t s, int32_t mx, unsigned long long ab, unsigned long long sq)
{
  if (!ab)
    return;  // (then mx and sq are zero as well)
  atomicMax(f.rmax + s, mx);
  atomicAdd(f.rsum + s, ab);
  atomicAdd(f.rsq + s, sq);
}

__global__ __launch_bounds__(FIT_THREADS) void residuals_kernel(const int32_t* __restrict__ xyz, int64_t n,
                                                                const int32_t* __restrict__ plane, int32_t npl, Fit f,
                                                                int32_t* __restrict__ residual)
{
  __shared__ int32_t s_max[FIT_CAP];
  __shared__ unsigned long long s_abs[FIT_CAP], s_sq[FIT_CAP];
  const int cap = min(npl, FIT_CAP);
  for (int k = threadIdx.x; k < cap; k += FIT_THREADS) {
    s_max[k] = 0;
    s_abs[k] = s_sq[k] = 0;
  }
  __syncthreads();
  const int64_t tile = (int64_t)FIT_THREADS * FIT_ITEMS;
  for (int64_t base = blockIdx.x * tile; base < n; base += gridDim.x * tile) {
    Pts p;
    load_points(xyz, n, plane, npl, base, p);
#pragma unroll
    for (int j = 0; j < FIT_ITEMS; j++) {
      const int64_t i = base + j * FIT_THREADS + threadIdx.x;
      int32_t s = p.s[j], r = INT32_MIN;
      if (s >= 0) {
        const int4 c = f.cen[s];
        if (c.w != 0) {
          s = -1;
        } else {
          const V3 nv = {f.normal[3 * s], f.normal[3 * s + 1], f.normal[3 * s + 2]};
          const V3 d = {(double)(p.x[j] - c.x), (double)(p.y[j] - c.y), (double)(p.z[j] - c.z)};
          r = (int32_t)(int64_t)dot_tree(nv, d);
        }
      }
      if (residual && i < n)
        residual[i] = r;
      const unsigned long long labelled = __ballot(s >= 0);
      if (!labelled)
        continue;
      const int32_t ar = s >= 0 ? abs(r) : 0;
      const unsigned long long ab = (unsigned long long)ar, sq = ab * ab;
      int32_t s0;
      if (wave_one_label(s, labelled, &s0)) {
        const int32_t mx = wave_max(ar);
        const unsigned long long wab = wave_sum(ab), wsq = wave_sum(sq);
        if ((threadIdx.x & 63) == 0) {
          if (s0 < FIT_CAP) {
            atomicMax(s_max + s0, mx);
            atomicAdd(s_abs + s0, wab);
            atomicAdd(s_sq + s0, wsq);
          } else {
            residuals_global(f, s0, mx, wab, wsq);
          }
        }
      } else if (s >= 0) {
        if (s < FIT_CAP) {
          atomicMax(s_max + s, ar);
          atomicAdd(s_abs + s, ab);
          atomicAdd(s_sq + s, sq);
        } else {
          residuals_global(f, s, ar, ab, sq);
        }
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < cap; k += FIT_THREADS)
    residuals_global(f, k, s_max[k], s_abs[k], s_sq[k]);
}

bool alloc_fits(struct bs_plane_fits* r, int32_t npl)
{
  const size_t m = (size_t)std::max(npl, 1);
  r->status = (int32_t*)calloc(m, 4);
  r->n_points = (int64_t*)calloc(m, 8);
  r->center = (int32_t*)calloc(3 * m, 4);
  r->normal = (double*)calloc(3 * m, 8);
  r->bbox = (int32_t*)calloc(6 * m, 4);
  r->dev_sum = (int64_t*)calloc(3 * m, 8);
  r->moment = (int64_t*)calloc(6 * m, 8);
  r->r_abs_max = (int32_t*)calloc(m, 4);
  r->r_abs_sum = (int64_t*)calloc(m, 8);
  r->r_sq_sum = (int64_t*)calloc(m, 8);
  return r->status && r->n_points && r->center && r->normal && r->bbox && r->dev_sum && r->moment && r->r_abs_max &&
         r->r_abs_sum && r->r_sq_sum;
}

const char* const FIT_INVALID = "plane fit: null pointer, n < 1 or n_planes < 0";

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_plane_fits_free(struct bs_plane_fits* r)
{
  if (!r)
    return;
  free(r->status);
  free(r->n_points);
  free(r->center);
  free(r->normal);
  free(r->bbox);
  free(r->dev_sum);
  free(r->moment);
  free(r->r_abs_max);
  free(r->r_abs_sum);
  free(r->r_sq_sum);
  memset(r, 0, sizeof *r);
}

extern "C" int bs_plane_fit_apply(const struct bs_plane_fits* f, double* normal, int32_t* center)
{
  if (!f || f->n_planes < 0 || (f->n_planes > 0 && (!normal || !center || !f->status || !f->normal || !f->center)))
    return BS_ERR_INVALID;
  for (int32_t p = 0; p < f->n_planes; p++) {
    if (f->status[p] != 0)
      continue;
    for (int a = 0; a < 3; a++) {
      normal[3 * p + a] = f->normal[3 * p + a];
      center[3 * p + a] = f->center[3 * p + a];
    }
  }
  return BS_OK;
}

extern "C" int bs_plane_fit_dev(bs_ctx* ctx, const int32_t* d_xyz, int64_t n, const int32_t* d_plane_idx,
                                int32_t n_planes, int32_t* d_residual, struct bs_plane_fits* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!d_xyz || !d_plane_idx || !out || n < 1 || n_planes < 0)
    return fail(ctx, BS_ERR_INVALID, FIT_INVALID);
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "plane fit: 2^29 points or more");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int32_t npl = n_planes;
  const size_t m = (size_t)std::max(npl, 1);
  DevBuf* B = ctx->ft;
  Events<6> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));
  BS_HIP(ctx, B[FT_TAB].reserve(FIT_BYTES * m));
  BS_HIP(ctx, B[FT_MISC].reserve(256));
  Fit f;
  f.cnt = B[FT_TAB].as<unsigned long long>();
  f.sum = f.cnt + m;
  f.mom = f.sum + 3 * m;
  f.rsum = f.mom + 6 * m;
  f.rsq = f.rsum + m;
  f.dev = reinterpret_cast<long long*>(f.rsq + m);
  f.normal = reinterpret_cast<double*>(f.dev + 3 * m);
  f.cen = reinterpret_cast<int4*>(f.normal + 3 * m);  // (144 m bytes in: 16-byte aligned)
  f.box = reinterpret_cast<int32_t*>(f.cen + m);
  f.rmax = f.box + 6 * m;
  int* d_bad = B[FT_MISC].as<int>();
  const int grid = (int)std::min<int64_t>(nblk(n, FIT_THREADS * FIT_ITEMS), FIT_GRID), pgrid = nblk(m, 256);

  // ---- sums, centroid and verdict ----
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  fit_init_kernel<<<pgrid, 256, 0, st>>>(f, (int32_t)m, d_bad);
  sums_kernel<<<grid, FIT_THREADS, 0, st>>>(d_xyz, n, d_plane_idx, npl, f, d_bad);
  verdict_kernel<<<pgrid, 256, 0, st>>>(f, npl);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  int h_bad = 0;  // (before anything is written to the caller's arrays)
  BS_HIP(ctx, hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_bad)
    return fail(ctx, BS_ERR_RANGE, "plane fit: coordinates must satisfy |c| < 2^23 mm: shift the cloud to its "
                                   "bounding-box origin first");

  // ---- moments ----
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));  // (the host looked at the flag in between)
  moments_kernel<<<grid, FIT_THREADS, 0, st>>>(d_xyz, n, d_plane_idx, npl, f);
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  // ---- solve ----
  solve_kernel<<<pgrid, 256, 0, st>>>(f, npl);
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  // ---- residuals ----
  residuals_kernel<<<grid, FIT_THREADS, 0, st>>>(d_xyz, n, d_plane_idx, npl, f, d_residual);
  BS_HIP(ctx, hipEventRecord(ev.e[5], st));

  struct bs_plane_fits r;
  memset(&r, 0, sizeof r);
  std::vector<int32_t> cen;
  try {
    cen.resize(4 * m);
  } catch (...) {
    return fail(ctx, BS_ERR_NOMEM, "plane fit: host allocation");
  }
  if (!alloc_fits(&r, npl)) {
    bs_plane_fits_free(&r);
    return fail(ctx, BS_ERR_NOMEM, "plane fit: host allocation");
  }
  hipError_t e = hipSuccess;
  auto fetch = [&](void* dst, const void* src, size_t bytes) {
    if (e == hipSuccess && npl > 0)
      e = hipMemcpyAsync(dst, src, bytes * (size_t)npl, hipMemcpyDeviceToHost, st);
  };
  fetch(r.n_points, f.cnt, 8);
  fetch(cen.data(), f.cen, 16);
  fetch(r.normal, f.normal, 24);
  fetch(r.bbox, f.box, 24);
  fetch(r.dev_sum, f.dev, 24);
  fetch(r.moment, f.mom, 48);
  fetch(r.r_abs_max, f.rmax, 4);
  fetch(r.r_abs_sum, f.rsum, 8);
  fetch(r.r_sq_sum, f.rsq, 8);
  if (e == hipSuccess)
    e = hipStreamSynchronize(st);
  if (e == hipSuccess)
    e = hipGetLastError();
  if (e != hipSuccess) {
    bs_plane_fits_free(&r);
    return fail(ctx, BS_ERR_HIP, "plane fit: results", e);
  }
  for (int32_t p = 0; p < npl; p++) {
    r.center[3 * p] = cen[4 * p];
    r.center[3 * p + 1] = cen[4 * p + 1];
    r.center[3 * p + 2] = cen[4 * p + 2];
    r.status[p] = cen[4 * p + 3];
  }
  r.n_planes = npl;
  r.ms_sums = ev.ms(0, 1);
  r.ms_moments = ev.ms(2, 3);
  r.ms_solve = ev.ms(3, 4);
  r.ms_residuals = ev.ms(4, 5);
  *out = r;
  return BS_OK;
}

extern "C" int bs_plane_fit(bs_ctx* ctx, const int32_t* xyz, int64_t n, const int32_t* plane_idx, int32_t n_planes,
                            int32_t* residual, struct bs_plane_fits* out)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!xyz || !plane_idx || !out || n < 1 || n_planes < 0)
    return fail(ctx, BS_ERR_INVALID, FIT_INVALID);
  if (n >= (1ll << 29))
    return fail(ctx, BS_ERR_RANGE, "plane fit: 2^29 points or more");
  DevBuf* B = ctx->ft;
  Staging S(ctx);
  const int32_t* d_xyz = S.upload(B[FT_IN_XYZ], xyz, 3 * (size_t)n);
  const int32_t* d_plane = S.upload(B[FT_IN_PLANE], plane_idx, (size_t)n);
  int32_t* d_res = S.room<int32_t>(B[FT_OUT], (size_t)n, residual != nullptr);
  if (!S.ok())
    return S.status();
  struct bs_plane_fits r;  // (out is written at the end alone: an error leaves it untouched)
  int rc = bs_plane_fit_dev(ctx, d_xyz, n, d_plane, n_planes, d_res, &r);
  if (rc != BS_OK)
    return rc;
  FreeUnlessKept<struct bs_plane_fits, bs_plane_fits_free> guard{&r};
  S.download(residual, d_res, (size_t)n);
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  *out = r;
  return BS_OK;
}
