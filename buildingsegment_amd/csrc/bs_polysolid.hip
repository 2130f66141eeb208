// bs_polysolid.hip -- polygon solids: a closed mesh per building (roof, floor, walls) over the clean vertices and the outline
// triangles (DESIGN.md "Polygon solids"; the definition is written down in include/bs_api.h under "polygon solids").
//   input     bs_outline_triangles_count_dev on the same images: the clean vertices with Z and right label, the ring of every
//             vertex, the first vertex of every ring (bs_ctx::uc_*) and the triangles (bs_ctx::tr_tri) stay on the device; the
//             host holds the rings' labels, tri_offset and label_status, reads label_building once and uploads per label its
//             building (-1: open, the label contributes nothing), its first vertex and the triangles up to and including it
//   twins     one 64-bit key (lower corner << 32 | higher corner) per clean segment that has one of its own building on its
//             right, ~0 for the rest; one radix sort; sorted positions 2 k and 2 k + 1 must be a pair
//   vertices  two entries (building, corner, Z) per clean vertex of a closed building -- its own Z and base_z; two stable
//             radix sorts (Z, then building << 32 | corner), head flags, one exclusive sum: every entry gets its vertex
//             number; the vertices of a column are consecutive, so "strictly between" is a difference of two numbers
//   count     per clean vertex the wall of its segment (exists, emitter, vertices, crossing) and the figures of its building;
//             per triangle the area and the volume; two exclusive sums over the walls
//   emit      per mesh vertex one 16-byte store; per triangle roof and floor; per emitting segment its wall
// The per-building figures are reduced as bs_solid.hip reduces its own: a wave inside one building in registers, buildings
// below FIG_CAP through LDS tables, the rest by global atomics.  Every index read from memory is checked before it is used
// as an address; a violation sets err and the call returns BS_ERR_INTERNAL.
// The label of a triangle slot (last_le, label_of_slot) is bs_trispan.h's, shared with the model raster and the point
// residuals; tri_of is this file's own, since a slot of a contributing label is never -1.  The entry points own the results
// of the stages before through bs_chain.h's Chain and hand them over at their end; an early return frees them.
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
#include "bs_trispan.h"  // (last_le, label_of_slot, Z_LIMIT)

namespace bs {
namespace {

// scratch of bs_ctx::ps
enum { PS_MISC, PS_TMP, PS_LC, PS_LV0, PS_TB2, PS_TOFF, PS_RLABEL, PS_TK0, PS_TK1, PS_TV0, PS_TV1, PS_TWIN, PS_ZK0, PS_ZK1, PS_EV0,
       PS_EV1, PS_EV2, PS_CK0, PS_CK1, PS_HEAD, PS_HSCAN, PS_VNUM, PS_VSRC, PS_WCNT, PS_WSCAN, PS_ISCAN, PS_FIG, PS_IN_LB, PS_OUT,
       PS_COUNT };
static_assert(PS_COUNT <= (int)(sizeof(bs_ctx::ps) / sizeof(DevBuf)), "bs_ctx::ps is too short");

constexpr int FIG_CAP = BS_POLY_FIG_CAP;  // buildings 0 .. FIG_CAP - 1: figures reduced in LDS (20 KiB in ps_wall_kernel)
constexpr unsigned long long NONE = ~0ull;
enum { W_ERR, W_RANGE, W_COUNT };                                               // the words of PS_MISC
enum { E_RING = 1, E_LABEL = 2, E_TWIN = 4, E_VNUM = 8, E_TRI = 16, E_EMIT = 32 };  // the bits of W_ERR

struct In {  // what the stages before left on the device, and the per-label words of the host
  const int2* xy;
  const int32_t* z;
  const int32_t* right;
  const int32_t* ring;
  const int32_t* soff;
  const int32_t* rlabel;  // the label of every ring
  const int32_t* lc;      // per label: its building, -1 if that is open
  const int32_t* lv0;     // per label: its first clean vertex
  const long long* tb2;   // per label: the triangles of the contributing labels up to and including it
  const long long* toff;  // tri_offset [n_labels + 1]
  const int32_t* tri;
  int32_t nsv, nr, nl, w1;  // (w1 = width + 1: a corner's index is Y * w1 + X)
  int32_t base, bin;
  long long ntri;
  // per-building bases (bs_set_building_bases): the table, nullptr while the switch is off; for the range check of the count
  // the buildings of the labels as the caller gave them (those of an open building too) and their number
  const int32_t* bases;
  const int32_t* lb;
  int32_t nb;
};

// base_z of building c, a checked building number
__device__ inline int32_t base_of(const In& A, int32_t c) { return A.bases ? A.bases[c] : A.base; }

struct Fig {  // per building, device
  unsigned long long *walls, *crossing, *area2, *volume6;
  unsigned* max_wall;
  int32_t *z_min, *z_max;
  unsigned *v_first, *v_end;
};

__device__ inline int32_t next_of(const In& A, int32_t i, int32_t r) { return i + 1 < A.soff[r + 1] ? i + 1 : A.soff[r]; }

// the label and the building of clean vertex i, its ring checked; c = -1 where the vertex contributes nothing
__device__ inline bool vertex_of(const In& A, int32_t i, int32_t& r, int32_t& l, int32_t& c, int* err)
{
  r = A.ring[i];
  if ((uint32_t)r >= (uint32_t)A.nr) {
    atomicOr(err, E_RING);
    return false;
  }
  l = A.rlabel[r];
  if ((uint32_t)l >= (uint32_t)A.nl) {
    atomicOr(err, E_LABEL);
    return false;
  }
  c = A.lc[l];
  const int32_t a = A.soff[r], b = A.soff[r + 1];
  if (a < 0 || a > i || b <= i || b > A.nsv) {
    atomicOr(err, E_RING);
    return false;
  }
  return true;
}

// ---- 1. twins, and the keys of the vertex entries -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ps_keys_kernel(In A, unsigned long long* __restrict__ tk, int32_t* __restrict__ tv,
                                                      int32_t* __restrict__ twin, uint32_t* __restrict__ zk,
                                                      uint32_t* __restrict__ ev, unsigned long long* __restrict__ ck,
                                                      int* __restrict__ words)
{
  for (int64_t i64 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i64 < A.nsv; i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    int32_t r, l, c = -1;
    unsigned long long key = NONE, col = NONE;
    const int32_t z = A.z[i];
    const bool known = vertex_of(A, i, r, l, c, words + W_ERR);
    // the base the vertex is measured against: under the switch that of its label's building, open or not (the host has
    // checked the table of the labels; a vertex without a ring or a label is an internal error and measured against nothing)
    long long base = A.base;
    bool measured = true;
    if (A.bases) {
      const int32_t b = known ? A.lb[l] : -1;
      measured = (uint32_t)b < (uint32_t)A.nb;
      if (measured)
        base = A.bases[b];
    }
    if (measured && ((long long)z - base >= Z_LIMIT || (long long)z - base <= -Z_LIMIT))
      atomicOr(words + W_RANGE, 1);
    if (known && c >= 0) {
      const int2 p = A.xy[i], q = A.xy[next_of(A, i, r)];
      const uint32_t ci = (uint32_t)p.y * (uint32_t)A.w1 + (uint32_t)p.x, cj = (uint32_t)q.y * (uint32_t)A.w1 + (uint32_t)q.x;
      col = ((unsigned long long)(uint32_t)c << 32) | ci;
      const int32_t R = A.right[i];
      if (R >= A.nl)
        atomicOr(words + W_ERR, E_LABEL);
      else if (R >= 0 && A.lc[R] == c)
        key = ((unsigned long long)min(ci, cj) << 32) | max(ci, cj);
    }
    tk[i] = key;
    tv[i] = i;
    twin[i] = -1;
    const uint32_t e = 2u * (uint32_t)i;
    zk[e] = (uint32_t)z ^ 0x80000000u;
    zk[e + 1] = (uint32_t)(known && c >= 0 ? base_of(A, c) : A.base) ^ 0x80000000u;
    ev[e] = e;
    ev[e + 1] = e + 1;
    ck[e] = ck[e + 1] = col;
  }
}

__global__ __launch_bounds__(256) void ps_twins_kernel(In A, const unsigned long long* __restrict__ tk, const int32_t* __restrict__ tv,
                                                       int32_t* __restrict__ twin, int* __restrict__ err)
{
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < A.nsv; p += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = tk[p];
    if (key == NONE)
      continue;
    const int64_t q = p ^ 1;
    if (q >= A.nsv || tk[q] != key) {
      atomicOr(err, E_TWIN);
      continue;
    }
    const int32_t i = tv[p], j = tv[q];
    if ((uint32_t)i >= (uint32_t)A.nsv || (uint32_t)j >= (uint32_t)A.nsv) {
      atomicOr(err, E_TWIN);
      continue;
    }
    int32_t ri, li, ci, rj, lj, cj;
    if (!vertex_of(A, i, ri, li, ci, err) || !vertex_of(A, j, rj, lj, cj, err))
      continue;
    const int2 is = A.xy[i], ie = A.xy[next_of(A, i, ri)], js = A.xy[j], je = A.xy[next_of(A, j, rj)];
    if (A.right[i] != lj || A.right[j] != li || is.x != je.x || is.y != je.y || ie.x != js.x || ie.y != js.y) {
      atomicOr(err, E_TWIN);
      continue;
    }
    twin[i] = j;
  }
}

// ---- 2. vertices ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ps_gather_kernel(const uint32_t* __restrict__ ev, const unsigned long long* __restrict__ ck,
                                                        int64_t m, unsigned long long* __restrict__ ck_sorted, int* __restrict__ err)
{
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t e = ev[p];
    if (e >= (uint64_t)m) {
      atomicOr(err, E_VNUM);
      ck_sorted[p] = NONE;
    } else {
      ck_sorted[p] = ck[e];
    }
  }
}

// (the entries are sorted by (column, Z): zk[ev[p]] is the Z key of position p)
__global__ __launch_bounds__(256) void ps_heads_kernel(const unsigned long long* __restrict__ ck, const uint32_t* __restrict__ ev,
                                                       const uint32_t* __restrict__ zk, int64_t m, uint32_t* __restrict__ head,
                                                       int* __restrict__ err)
{
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p <= m; p += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = 0;
    if (p < m && ck[p] != NONE) {
      const uint32_t e = ev[p], e0 = p > 0 ? ev[p - 1] : 0;
      if (e >= (uint64_t)m || e0 >= (uint64_t)m)
        atomicOr(err, E_VNUM);
      else
        h = p == 0 || ck[p - 1] != ck[p] || zk[e0] != zk[e];
    }
    head[p] = h;
  }
}

__global__ __launch_bounds__(256) void ps_numbers_kernel(const unsigned long long* __restrict__ ck, const uint32_t* __restrict__ ev,
                                                         const uint32_t* __restrict__ head, const uint32_t* __restrict__ hscan,
                                                         int64_t m, int32_t nb, int32_t* __restrict__ vnum, int32_t* __restrict__ vsrc,
                                                         Fig f, int* __restrict__ err)
{
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < m; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t e = ev[p];
    if (e >= (uint64_t)m) {
      atomicOr(err, E_VNUM);
      continue;
    }
    const unsigned long long k = ck[p];
    if (k == NONE) {
      vnum[e] = -1;
      continue;
    }
    const uint32_t c = (uint32_t)(k >> 32), v = hscan[p] + head[p] - 1u;
    if (c >= (uint32_t)nb || v >= (uint64_t)m) {
      atomicOr(err, E_VNUM);
      continue;
    }
    vnum[e] = (int32_t)v;
    if (head[p])
      vsrc[v] = (int32_t)e;
    // the vertices of a building are one run of the sorted order
    if (p == 0 || (uint32_t)(ck[p - 1] >> 32) != c)
      f.v_first[c] = v;
    if (p + 1 == m || ck[p + 1] == NONE || (uint32_t)(ck[p + 1] >> 32) != c)
      f.v_end[c] = v + 1u;
  }
}

// ---- 3. count -------------------------------------------------------------------------------------------------------------
struct Wall {
  int32_t va_s, va_e, vb_s, vb_e;  // vertex numbers
  int32_t ds, de;                  // steps down (or up) the two columns
  bool emit, crossing;
};

// the wall of the segment that starts at clean vertex i of ring r, label l, building c >= 0
__device__ inline bool wall_of(const In& A, const int32_t* __restrict__ twin, const int32_t* __restrict__ vnum, int32_t i, int32_t r,
                               int32_t l, Wall& w, int* err)
{
  const int32_t e = next_of(A, i, r), t = twin[i];
  int32_t bs = base_of(A, A.lc[l]), be = bs;
  w.va_s = vnum[2 * (int64_t)i];
  w.va_e = vnum[2 * (int64_t)e];
  w.emit = true;
  if (t >= 0) {
    int32_t rt, lt, ct;
    if (t >= A.nsv || !vertex_of(A, t, rt, lt, ct, err))
      return false;
    const int32_t nt = next_of(A, t, rt);
    w.vb_e = vnum[2 * (int64_t)t];
    w.vb_s = vnum[2 * (int64_t)nt];
    be = A.z[t];
    bs = A.z[nt];
    w.emit = l < lt;
  } else {
    w.vb_s = vnum[2 * (int64_t)i + 1];
    w.vb_e = vnum[2 * (int64_t)e + 1];
  }
  if ((w.va_s | w.va_e | w.vb_s | w.vb_e) < 0) {
    atomicOr(err, E_VNUM);
    return false;
  }
  w.ds = abs(w.va_s - w.vb_s);
  w.de = abs(w.va_e - w.vb_e);
  const long long gs = (long long)A.z[i] - bs, ge = (long long)A.z[e] - be;
  w.crossing = (gs < 0 && ge > 0) || (gs > 0 && ge < 0);
  if ((w.ds == 0) != (gs == 0) || (w.de == 0) != (ge == 0) || w.ds > 64 || w.de > 64) {  // (a column holds a handful)
    atomicOr(err, E_VNUM);
    return false;
  }
  return true;
}

__device__ inline void fig_walls(const Fig& f, int32_t c, unsigned walls, unsigned cross, unsigned mw, int32_t mn, int32_t mx)
{
  if (walls)
    atomicAdd(f.walls + c, (unsigned long long)walls);
  if (cross)
    atomicAdd(f.crossing + c, (unsigned long long)cross);
  if (mw)
    atomicMax(f.max_wall + c, mw);
  atomicMin(f.z_min + c, mn);
  atomicMax(f.z_max + c, mx);
}

__global__ __launch_bounds__(256) void ps_wall_kernel(In A, const int32_t* __restrict__ twin, const int32_t* __restrict__ vnum,
                                                      int32_t nb, int32_t* __restrict__ wcnt, Fig f, int* __restrict__ err)
{
  __shared__ unsigned s_walls[FIG_CAP], s_cross[FIG_CAP], s_mw[FIG_CAP];
  __shared__ int s_mn[FIG_CAP], s_mx[FIG_CAP];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x) {
    s_walls[k] = s_cross[k] = s_mw[k] = 0;
    s_mn[k] = INT32_MAX;
    s_mx[k] = INT32_MIN;
  }
  __syncthreads();
  const int64_t n64 = ((int64_t)A.nsv + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i64 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i64 < n64; i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64;
    int32_t r, l, c = -1;
    unsigned walls = 0, cross = 0, mw = 0;
    int32_t mn = INT32_MAX, mx = INT32_MIN;
    if (i64 < A.nsv) {
      int32_t cnt = 0;
      if (vertex_of(A, i, r, l, c, err) && c >= 0) {
        if (c >= nb) {
          atomicOr(err, E_LABEL);
          c = -1;
        } else {
          Wall w;
          if (wall_of(A, twin, vnum, i, r, l, w, err) && w.emit && w.ds + w.de > 0) {
            cnt = 2 + w.ds + w.de;
            walls = 1;
            cross = w.crossing;
            mw = (unsigned)cnt;
          }
          mn = mx = A.z[i];
        }
      }
      wcnt[i] = cnt;
    }
    const int32_t c0 = __shfl(c, 0);
    if (__all(c == c0)) {  // the whole wave inside one building (or in none): reduce in registers
      if (c0 < 0)
        continue;
      for (int o = 32; o > 0; o >>= 1) {
        walls += __shfl_xor(walls, o);
        cross += __shfl_xor(cross, o);
        mw = max(mw, __shfl_xor(mw, o));
        mn = min(mn, __shfl_xor(mn, o));
        mx = max(mx, __shfl_xor(mx, o));
      }
      if ((threadIdx.x & 63) == 0) {
        if (c0 < FIG_CAP) {
          atomicAdd(s_walls + c0, walls);
          atomicAdd(s_cross + c0, cross);
          atomicMax(s_mw + c0, mw);
          atomicMin(s_mn + c0, mn);
          atomicMax(s_mx + c0, mx);
        } else {
          fig_walls(f, c0, walls, cross, mw, mn, mx);
        }
      }
    } else if (c >= 0) {
      if (c < FIG_CAP) {
        if (walls)
          atomicAdd(s_walls + c, walls);
        if (cross)
          atomicAdd(s_cross + c, cross);
        if (mw)
          atomicMax(s_mw + c, mw);
        atomicMin(s_mn + c, mn);
        atomicMax(s_mx + c, mx);
      } else {
        fig_walls(f, c, walls, cross, mw, mn, mx);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x)
    if (s_mn[k] <= s_mx[k])
      fig_walls(f, k, s_walls[k], s_cross[k], s_mw[k], s_mn[k], s_mx[k]);
}

// the three clean vertices of slot q of a contributing label (so never a slot of -1, unlike bs_trispan.h's), checked
__device__ inline bool tri_of(const In& A, long long q, int32_t& a, int32_t& b, int32_t& d, int* err)
{
  a = A.tri[3 * q];
  b = A.tri[3 * q + 1];
  d = A.tri[3 * q + 2];
  if ((uint32_t)a >= (uint32_t)A.nsv || (uint32_t)b >= (uint32_t)A.nsv || (uint32_t)d >= (uint32_t)A.nsv) {
    atomicOr(err, E_TRI);
    return false;
  }
  return true;
}

__global__ __launch_bounds__(256) void ps_tri_kernel(In A, int32_t nb, Fig f, int* __restrict__ err)
{
  __shared__ unsigned long long s_area[FIG_CAP], s_vol[FIG_CAP];
  for (int k = threadIdx.x; k < FIG_CAP; k += blockDim.x)
    s_area[k] = s_vol[k] = 0;
  __syncthreads();
  const long long n64 = (A.ntri + 63) & ~63ll;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < n64; q += (long long)gridDim.x * blockDim.x) {
    int32_t c = -1;
    unsigned long long area = 0, vol = 0;
    if (q < A.ntri) {
      const int32_t l = label_of_slot(A.toff, A.nl, q);
      int32_t a, b, d;
      c = A.lc[l];
      if (c >= nb) {
        atomicOr(err, E_LABEL);
        c = -1;
      }
      if (c >= 0 && tri_of(A, q, a, b, d, err)) {
        const int2 pa = A.xy[a], pb = A.xy[b], pd = A.xy[d];
        const long long o = (long long)(pb.x - pa.x) * (pd.y - pa.y) - (long long)(pb.y - pa.y) * (pd.x - pa.x);
        area = (unsigned long long)o;
        vol = (unsigned long long)(o * ((long long)A.z[a] + A.z[b] + A.z[d] - 3ll * base_of(A, c)));
      } else {
        c = -1;
      }
    }
    const int32_t c0 = __shfl(c, 0);
    if (__all(c == c0)) {
      if (c0 < 0)
        continue;
      for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_xor(area, o);
        vol += __shfl_xor(vol, o);
      }
      if ((threadIdx.x & 63) == 0) {
        atomicAdd((c0 < FIG_CAP ? s_area : f.area2) + c0, area);
        atomicAdd((c0 < FIG_CAP ? s_vol : f.volume6) + c0, vol);
      }
    } else if (c >= 0) {
      atomicAdd((c < FIG_CAP ? s_area : f.area2) + c, area);
      atomicAdd((c < FIG_CAP ? s_vol : f.volume6) + c, vol);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < FIG_CAP && k < nb; k += blockDim.x)
    if (s_area[k] | s_vol[k]) {
      atomicAdd(f.area2 + k, s_area[k]);
      atomicAdd(f.volume6 + k, s_vol[k]);
    }
}

__global__ __launch_bounds__(256) void ps_fig_init_kernel(Fig f, int32_t nb)
{
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < nb; c += (int64_t)gridDim.x * blockDim.x) {
    f.walls[c] = f.crossing[c] = f.area2[c] = f.volume6[c] = 0;
    f.max_wall[c] = f.v_first[c] = f.v_end[c] = 0;
    f.z_min[c] = INT32_MAX;
    f.z_max[c] = INT32_MIN;
  }
}

struct WallFlag {  // 0 for the entry behind the last
  const int32_t* wcnt;
  int32_t n;
  __host__ __device__ int32_t operator()(int32_t i) const { return i < n && wcnt[i] > 0; }
};
struct WallCount {
  const int32_t* wcnt;
  int32_t n;
  __host__ __device__ long long operator()(int32_t i) const { return i < n ? wcnt[i] : 0; }
};
using Idx = hipcub::CountingInputIterator<int32_t>;
using WallFlagIt = hipcub::TransformInputIterator<int32_t, WallFlag, Idx>;
using WallCountIt = hipcub::TransformInputIterator<long long, WallCount, Idx>;

// ---- 4. emit --------------------------------------------------------------------------------------------------------------
struct Mesh {
  int4* vertex;
  int32_t *offset, *index, *building;
  uint8_t* kind;
  long long nv, nf, ni;
};

__global__ __launch_bounds__(256) void ps_emit_vertex_kernel(In A, const int32_t* __restrict__ vsrc, Mesh o, int* __restrict__ err)
{
  for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < o.nv; v += (long long)gridDim.x * blockDim.x) {
    const int32_t e = vsrc[v], i = e >> 1;
    int32_t r, l, c;
    if ((uint32_t)i >= (uint32_t)A.nsv || !vertex_of(A, i, r, l, c, err) || c < 0) {
      atomicOr(err, E_EMIT);
      continue;
    }
    const int2 p = A.xy[i];
    o.vertex[v] = make_int4(p.x * A.bin, p.y * A.bin, (e & 1) ? base_of(A, c) : A.z[i], c);
  }
}

__global__ __launch_bounds__(256) void ps_emit_tri_kernel(In A, const int32_t* __restrict__ vnum, const int32_t* __restrict__ wscan,
                                                          const long long* __restrict__ iscan, Mesh o, int* __restrict__ err)
{
  if (blockIdx.x == 0 && threadIdx.x == 0)
    o.offset[o.nf] = (int32_t)o.ni;
  for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < A.ntri; q += (long long)gridDim.x * blockDim.x) {
    const int32_t l = label_of_slot(A.toff, A.nl, q), c = A.lc[l];
    int32_t a, b, d;
    if (c < 0 || !tri_of(A, q, a, b, d, err))
      continue;
    const long long T = A.toff[l + 1] - A.toff[l], j = q - A.toff[l], tb = A.tb2[l] - T;
    const int32_t v0 = A.lv0[l];
    if ((uint32_t)v0 >= (uint32_t)A.nsv || j < 0 || j >= T || tb < 0) {
      atomicOr(err, E_EMIT);
      continue;
    }
    const long long F = 2 * tb + wscan[v0], I = 6 * tb + iscan[v0];
    const long long f0 = F + j, f1 = F + T + j, i0 = I + 3 * j, i1 = I + 3 * T + 3 * j;
    const int32_t ra = vnum[2ll * a], rb = vnum[2ll * b], rd = vnum[2ll * d];
    const int32_t fa = vnum[2ll * a + 1], fb = vnum[2ll * b + 1], fd = vnum[2ll * d + 1];
    if (f1 >= o.nf || i1 + 3 > o.ni || (ra | rb | rd | fa | fb | fd) < 0) {
      atomicOr(err, E_EMIT);
      continue;
    }
    o.offset[f0] = (int32_t)i0;
    o.offset[f1] = (int32_t)i1;
    o.building[f0] = o.building[f1] = c;
    o.kind[f0] = 0;
    o.kind[f1] = 1;
    o.index[i0] = ra; o.index[i0 + 1] = rb; o.index[i0 + 2] = rd;
    o.index[i1] = fd; o.index[i1 + 1] = fb; o.index[i1 + 2] = fa;
  }
}

__global__ __launch_bounds__(256) void ps_emit_wall_kernel(In A, const int32_t* __restrict__ twin, const int32_t* __restrict__ vnum,
                                                           const int32_t* __restrict__ wcnt, const int32_t* __restrict__ wscan,
                                                           const long long* __restrict__ iscan, Mesh o, int* __restrict__ err)
{
  for (int64_t i64 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i64 < A.nsv; i64 += (int64_t)gridDim.x * blockDim.x) {
    const int32_t i = (int32_t)i64, cnt = wcnt[i];
    if (cnt <= 0)
      continue;
    int32_t r, l, c;
    Wall w;
    if (!vertex_of(A, i, r, l, c, err) || c < 0 || !wall_of(A, twin, vnum, i, r, l, w, err) || cnt != 2 + w.ds + w.de) {
      atomicOr(err, E_EMIT);
      continue;
    }
    const long long f = 2 * A.tb2[l] + wscan[i];
    long long k = 6 * A.tb2[l] + iscan[i];
    if (f < 0 || f >= o.nf || k < 0 || k + cnt > o.ni) {
      atomicOr(err, E_EMIT);
      continue;
    }
    o.offset[f] = (int32_t)k;
    o.building[f] = c;
    o.kind[f] = 2;
    o.index[k++] = w.va_e;
    o.index[k++] = w.va_s;
    const int32_t ss = w.vb_s > w.va_s ? 1 : -1, se = w.va_e > w.vb_e ? 1 : -1;
    for (int32_t j = 1; j <= w.ds; j++)  // the column of s from a_s, its end (s, b_s) included
      o.index[k++] = w.va_s + j * ss;
    for (int32_t j = 0; j < w.de; j++)  // the column of e from (e, b_e), its end (e, a_e) left out
      o.index[k++] = w.vb_e + j * se;
  }
}

using ResultGuard = FreeUnlessKept<struct bs_poly_solids, bs_poly_solids_free>;

int internal(bs_ctx* ctx, int err)
{
  char msg[112];
  snprintf(msg, sizeof msg, "polygon solids: a twin is missing or an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

const char* const PS_INVALID =
    "polygon solids: null pointer, no top image, n_buildings < 0 or bin < 1";

// the polygon solids over the triangles t of the clean outlines c, whose count has just run on ctx; res is zeroed
int poly_solids(bs_ctx* ctx, const struct bs_outline_triangles& t, const struct bs_clean_outlines& c, int32_t width,
                const int32_t* d_label_building, int32_t nb, int32_t bin, int32_t base_z, struct bs_poly_solids& res)
{
  const int32_t nl = c.n_labels, nr = (int32_t)c.n_rings, nsv = (int32_t)c.n_svertices;
  const int64_t ntri = t.n_triangles, m = 2 * (int64_t)nsv;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->ps;
  // ---- the host's part: the buildings of the labels, which are open, the per-label words ----
  std::vector<int32_t> lb((size_t)std::max(nl, 1));
  if (nl > 0) {
    BS_HIP(ctx, hipMemcpyAsync(lb.data(), d_label_building, 4 * (size_t)nl, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
  }
  for (int32_t l = 0; l < nl; l++)
    if (lb[l] < 0 || lb[l] >= nb)
      return fail(ctx, BS_ERR_RANGE, "polygon solids: a label_building value outside 0 .. n_buildings - 1");
  res.n_buildings = nb;
  res.n_labels = nl;
  res.bin = bin;
  res.base_z = base_z;
  res.fig_cap = FIG_CAP;
  res.ms_triangles = t.ms_clean + t.ms_prologue + t.ms_wave + t.ms_lds + t.ms_global;
  const size_t nbs = (size_t)nb;
  const bool ok[] = {alloc(&res.status, nbs),     alloc(&res.labels, nbs),         alloc(&res.vertices, nbs),
                     alloc(&res.faces, nbs),      alloc(&res.roof_faces, nbs),     alloc(&res.wall_faces, nbs),
                     alloc(&res.crossing_walls, nbs), alloc(&res.max_wall_vertices, nbs), alloc(&res.z_min, nbs),
                     alloc(&res.z_max, nbs),      alloc(&res.area2, nbs),          alloc(&res.volume6, nbs)};
  if (!std::all_of(std::begin(ok), std::end(ok), [](bool b) { return b; }))
    return fail(ctx, BS_ERR_NOMEM, "polygon solids: host allocation");
  for (int32_t b = 0; b < nb; b++) {
    res.z_min[b] = INT32_MAX;
    res.z_max[b] = INT32_MIN;
  }
  for (int32_t l = 0; l < nl; l++) {
    res.labels[lb[l]]++;
    if (t.label_status[l] == BS_TRI_NO_BRIDGE || t.label_status[l] == BS_TRI_STALLED)
      res.status[lb[l]] = 1;
  }
  for (int32_t b = 0; b < nb; b++)
    res.n_open_buildings += res.status[b];
  std::vector<int32_t> lc((size_t)std::max(nl, 1)), lv0((size_t)std::max(nl, 1)), rlabel((size_t)std::max(nr, 1));
  std::vector<long long> tb2((size_t)std::max(nl, 1)), toff((size_t)nl + 1);
  long long tb = 0;
  for (int32_t l = 0; l < nl; l++) {
    const int64_t r0 = c.label_ring_offset[l];
    lc[l] = res.status[lb[l]] ? -1 : lb[l];
    lv0[l] = (int32_t)std::min<int64_t>(c.s_ring_offset[r0], std::max(nsv - 1, 0));
    toff[l] = t.tri_offset[l];
    if (lc[l] >= 0 && t.label_status[l] == BS_TRI_OK) {
      const long long T = t.tri_offset[l + 1] - t.tri_offset[l];
      tb += T;
      res.roof_faces[lb[l]] += T;
    }
    tb2[l] = tb;
  }
  toff[nl] = t.tri_offset[nl];
  for (int32_t r = 0; r < nr; r++)
    rlabel[r] = c.ring_label[r];
  res.n_roof_faces = tb;
  ctx->ps_bin = bin;
  ctx->ps_base = base_z;
  const int32_t* d_bases = nullptr;
  if (const int rc = building_bases(ctx, nb, "polygon solids", &d_bases))
    return rc;
  ctx->ps_bases = d_bases != nullptr;
  ctx->ps_nl = nl;
  ctx->ps_nr = nr;
  ctx->ps_nsv = nsv;
  ctx->ps_ntri = ntri;
  ctx->ps_nv = ctx->ps_nf = ctx->ps_ni = 0;
  if (nsv == 0)  // no ring: an empty mesh
    return BS_OK;
  if (!ctx->uc_xy || !ctx->uc_z || !ctx->uc_right || !ctx->uc_ring || !ctx->uc_soff || (ntri > 0 && !ctx->tr_tri))
    return internal(ctx, 0x10000);
  // ---- device ----
  Events<4> ev;
  for (int i = 0; i < 4; i++)
    BS_HIP(ctx, hipEventCreate(&ev.e[i]));
  const int col_bits = std::min(64, 33 + bits_of(nb));  // (one bit above the building: ~0 sorts behind every column)
  BS_HIP(ctx, B[PS_MISC].reserve(256));
  for (int b : {PS_LC, PS_LV0})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)nl));
  BS_HIP(ctx, B[PS_TB2].reserve(8 * (size_t)nl));
  BS_HIP(ctx, B[PS_TOFF].reserve(8 * ((size_t)nl + 1)));
  BS_HIP(ctx, B[PS_RLABEL].reserve(4 * (size_t)nr));
  for (int b : {PS_TK0, PS_TK1})
    BS_HIP(ctx, B[b].reserve(8 * (size_t)nsv));
  for (int b : {PS_TV0, PS_TV1, PS_TWIN, PS_WCNT})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)nsv));
  for (int b : {PS_ZK0, PS_ZK1, PS_EV0, PS_EV1, PS_EV2, PS_VNUM, PS_VSRC})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)m));
  for (int b : {PS_CK0, PS_CK1})
    BS_HIP(ctx, B[b].reserve(8 * (size_t)m));
  for (int b : {PS_HEAD, PS_HSCAN})
    BS_HIP(ctx, B[b].reserve(4 * ((size_t)m + 1)));
  BS_HIP(ctx, B[PS_WSCAN].reserve(4 * ((size_t)nsv + 1)));
  BS_HIP(ctx, B[PS_ISCAN].reserve(8 * ((size_t)nsv + 1)));
  BS_HIP(ctx, B[PS_FIG].reserve(52 * nbs + 64));
  Fig f;
  f.walls = B[PS_FIG].as<unsigned long long>();
  f.crossing = f.walls + nbs;
  f.area2 = f.crossing + nbs;
  f.volume6 = f.area2 + nbs;
  f.max_wall = (unsigned*)(f.volume6 + nbs);
  f.z_min = (int32_t*)(f.max_wall + nbs);
  f.z_max = f.z_min + nbs;
  f.v_first = (unsigned*)(f.z_max + nbs);
  f.v_end = f.v_first + nbs;
  int* d_words = B[PS_MISC].as<int>();
  int* d_err = d_words + W_ERR;
  const In A{ctx->uc_xy, ctx->uc_z, ctx->uc_right, ctx->uc_ring, ctx->uc_soff, B[PS_RLABEL].as<int32_t>(), B[PS_LC].as<int32_t>(),
             B[PS_LV0].as<int32_t>(), B[PS_TB2].as<long long>(), B[PS_TOFF].as<long long>(), ctx->tr_tri, nsv, nr, nl, width + 1,
             base_z, bin, ntri, d_bases, d_label_building, nb};
  unsigned long long *tk0 = B[PS_TK0].as<unsigned long long>(), *tk1 = B[PS_TK1].as<unsigned long long>();
  int32_t *tv0 = B[PS_TV0].as<int32_t>(), *tv1 = B[PS_TV1].as<int32_t>(), *twin = B[PS_TWIN].as<int32_t>();
  uint32_t *zk0 = B[PS_ZK0].as<uint32_t>(), *zk1 = B[PS_ZK1].as<uint32_t>();
  uint32_t *ev0 = B[PS_EV0].as<uint32_t>(), *ev1 = B[PS_EV1].as<uint32_t>(), *ev2 = B[PS_EV2].as<uint32_t>();
  unsigned long long *ck0 = B[PS_CK0].as<unsigned long long>(), *ck1 = B[PS_CK1].as<unsigned long long>();
  uint32_t *head = B[PS_HEAD].as<uint32_t>(), *hscan = B[PS_HSCAN].as<uint32_t>();
  int32_t *vnum = B[PS_VNUM].as<int32_t>(), *vsrc = B[PS_VSRC].as<int32_t>(), *wcnt = B[PS_WCNT].as<int32_t>();
  int32_t* wscan = B[PS_WSCAN].as<int32_t>();
  long long* iscan = B[PS_ISCAN].as<long long>();
  auto sort = [st](auto* k0, auto* k1, auto* v0, auto* v1, auto n, int bits) {  // (n: int32 over the ring vertices, int64 over the entries, as ever)
    return [=](void* tmp, size_t& bytes) { return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, k0, k1, v0, v1, n, 0, bits, st); };
  };
  auto scan = [st](auto counts, auto* sums, auto n) {
    return [=](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, counts, sums, n, st); };
  };
  auto sort_twins = sort(tk0, tk1, tv0, tv1, nsv, 64);
  auto sort_z = sort(zk0, zk1, ev0, ev1, m, 32);
  auto sort_col = sort(ck1, ck0, ev1, ev2, m, col_bits);
  auto scan_heads = scan(head, hscan, m + 1);
  auto scan_walls = scan(WallFlagIt(Idx(0), WallFlag{wcnt, nsv}), wscan, nsv + 1);
  auto scan_index = scan(WallCountIt(Idx(0), WallCount{wcnt, nsv}), iscan, nsv + 1);
  BS_HIP(ctx, cub_room(B[PS_TMP], sort_twins, sort_z, sort_col, scan_heads, scan_walls, scan_index));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_words, 0, 4 * W_COUNT, st));
  BS_HIP(ctx, hipMemcpyAsync(B[PS_LC].p, lc.data(), 4 * (size_t)nl, hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[PS_LV0].p, lv0.data(), 4 * (size_t)nl, hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[PS_TB2].p, tb2.data(), 8 * (size_t)nl, hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[PS_TOFF].p, toff.data(), 8 * ((size_t)nl + 1), hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[PS_RLABEL].p, rlabel.data(), 4 * (size_t)nr, hipMemcpyHostToDevice, st));
  ps_fig_init_kernel<<<sweep(nb), 256, 0, st>>>(f, nb);
  // 1. twins (the keys of the vertex entries come out of the same pass)
  ps_keys_kernel<<<sweep(nsv), 256, 0, st>>>(A, tk0, tv0, twin, zk0, ev0, ck0, d_words);
  BS_HIP(ctx, cub_run(B[PS_TMP], sort_twins));
  ps_twins_kernel<<<sweep(nsv), 256, 0, st>>>(A, tk1, tv1, twin, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  // 2. vertices: two stable passes, Z first
  BS_HIP(ctx, cub_run(B[PS_TMP], sort_z));
  ps_gather_kernel<<<sweep(m), 256, 0, st>>>(ev1, ck0, m, ck1, d_err);
  BS_HIP(ctx, cub_run(B[PS_TMP], sort_col));
  ps_heads_kernel<<<sweep(m + 1), 256, 0, st>>>(ck0, ev2, zk0, m, head, d_err);
  BS_HIP(ctx, cub_run(B[PS_TMP], scan_heads));
  ps_numbers_kernel<<<sweep(m), 256, 0, st>>>(ck0, ev2, head, hscan, m, nb, vnum, vsrc, f, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  // 3. count
  ps_wall_kernel<<<sweep(nsv), 256, 0, st>>>(A, twin, vnum, nb, wcnt, f, d_err);
  if (ntri > 0)
    ps_tri_kernel<<<sweep(ntri), 256, 0, st>>>(A, nb, f, d_err);
  BS_HIP(ctx, cub_run(B[PS_TMP], scan_walls));
  BS_HIP(ctx, cub_run(B[PS_TMP], scan_index));
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  int h_words[W_COUNT] = {};
  uint32_t h_nv = 0;
  int32_t h_walls = 0;
  long long h_windices = 0;
  std::vector<char> h_fig(52 * nbs + 64);
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_COUNT, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&h_nv, hscan + m, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&h_walls, wscan + nsv, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&h_windices, iscan + nsv, 8, hipMemcpyDeviceToHost, st));
  if (nb > 0)
    BS_HIP(ctx, hipMemcpyAsync(h_fig.data(), B[PS_FIG].p, 52 * nbs, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  if (h_words[W_RANGE])
    return fail(ctx, BS_ERR_RANGE, "polygon solids: a clean vertex lies 2^24 or more above or below base_z");
  if (h_words[W_ERR])
    return internal(ctx, h_words[W_ERR]);
  const long long nf = 2 * tb + h_walls, ni = 6 * tb + h_windices;
  if (h_nv >= (1u << 31) || nf >= (1ll << 31) || ni >= (1ll << 31))
    return fail(ctx, BS_ERR_RANGE, "polygon solids: 2^31 or more vertices or indices");
  const unsigned long long* hw = (const unsigned long long*)h_fig.data();
  const unsigned* hm = (const unsigned*)(hw + 4 * nbs);
  const int32_t* hz = (const int32_t*)(hm + nbs);
  const unsigned* hv = (const unsigned*)(hz + 2 * nbs);
  for (int32_t b = 0; b < nb; b++) {
    res.wall_faces[b] = (int64_t)hw[b];
    res.crossing_walls[b] = (int64_t)hw[nbs + b];
    res.area2[b] = (int64_t)hw[2 * nbs + b];
    res.volume6[b] = (int64_t)hw[3 * nbs + b];
    res.max_wall_vertices[b] = (int64_t)hm[b];
    res.z_min[b] = hz[b];
    res.z_max[b] = hz[nbs + b];
    res.vertices[b] = (int64_t)hv[nbs + b] - (int64_t)hv[b];
    res.faces[b] = 2 * res.roof_faces[b] + res.wall_faces[b];
    res.n_wall_faces += res.wall_faces[b];
    res.n_crossing_walls += res.crossing_walls[b];
    res.max_wall_vertices_all = std::max(res.max_wall_vertices_all, res.max_wall_vertices[b]);
    res.total_area2 += res.area2[b];
    res.total_volume6 += res.volume6[b];
  }
  if (res.n_wall_faces != h_walls)
    return internal(ctx, 0x20000);
  res.n_vertices = h_nv;
  res.n_faces = nf;
  res.n_indices = ni;
  res.ms_twins = ev.ms(0, 1);
  res.ms_vertices = ev.ms(1, 2);
  res.ms_count = ev.ms(2, 3);
  ctx->ps_nv = h_nv;
  ctx->ps_nf = nf;
  ctx->ps_ni = ni;
  return BS_OK;
}

int check_args(bs_ctx* ctx, const void* label, const void* top, const void* lb, int32_t n_labels, int32_t nb, int32_t bin, const void* out)
{
  if (!label || !top || !out || (n_labels > 0 && !lb) || nb < 0 || bin < 1)
    return fail(ctx, BS_ERR_INVALID, PS_INVALID);
  const int32_t* d_bases;  // (a table of another length: refused before the stages in front run)
  return building_bases(ctx, nb, "polygon solids", &d_bases);
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_poly_solids_free(struct bs_poly_solids* s)
{
  if (!s)
    return;
  free(s->status);
  free(s->labels);
  free(s->vertices);
  free(s->faces);
  free(s->roof_faces);
  free(s->wall_faces);
  free(s->crossing_walls);
  free(s->max_wall_vertices);
  free(s->z_min);
  free(s->z_max);
  free(s->area2);
  free(s->volume6);
  free(s->vertex);
  free(s->face_offset);
  free(s->face_index);
  free(s->face_building);
  free(s->face_kind);
  memset(s, 0, sizeof *s);
}

extern "C" int bs_poly_solids_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                        int32_t n_labels, int64_t num, int64_t den, int32_t cell_log2,
                                        const int32_t* d_label_building, int32_t n_buildings, int32_t bin, int32_t base_z,
                                        struct bs_poly_solids* out, struct bs_outline_triangles* tri,
                                        struct bs_clean_outlines* clean, struct bs_simple_outlines* simple, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->ps_valid = false;
  int rc = check_args(ctx, d_label, d_top, d_label_building, n_labels, n_buildings, bin, out);
  if (rc != BS_OK)
    return rc;
  Chain ch;
  rc = bs_outline_triangles_count_dev(ctx, d_label, d_top, width, height, n_labels, num, den, cell_log2, &ch.tri, &ch.clean, &ch.simple,
                                      &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_tri = ch.has_clean = ch.has_simple = ch.has_plain = true;
  struct bs_poly_solids res;
  memset(&res, 0, sizeof res);
  ResultGuard guard{&res};
  rc = poly_solids(ctx, ch.tri, ch.clean, width, d_label_building, n_buildings, bin, base_z, res);
  if (rc != BS_OK)
    return rc;
  guard.keep = true;
  ch.hand_over(tri, clean, simple, plain);
  *out = res;
  ctx->ps_valid = true;
  return BS_OK;
}

extern "C" int bs_poly_solids_emit_dev(bs_ctx* ctx, int32_t* d_vertex, int32_t* d_face_offset, int32_t* d_face_index,
                                       int32_t* d_face_building, uint8_t* d_face_kind)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!ctx->ps_valid || !ctx->tr_valid || !ctx->uc_valid)
    return fail(ctx, BS_ERR_INVALID, "polygon solids: emit without a successful count on this context");
  const int64_t nv = ctx->ps_nv, nf = ctx->ps_nf, ni = ctx->ps_ni;
  if (!d_face_offset || (nv > 0 && !d_vertex) || (nf > 0 && (!d_face_index || !d_face_building || !d_face_kind)))
    return fail(ctx, BS_ERR_INVALID, "polygon solids: emit: null pointer");
  if (((uintptr_t)d_vertex & 15) != 0)
    return fail(ctx, BS_ERR_INVALID, "polygon solids: emit: d_vertex is not 16-byte aligned");
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  ctx->ps_ms_emit[0] = ctx->ps_ms_emit[1] = 0;
  if (ctx->ps_nsv == 0 || nv == 0) {  // an empty mesh: face_offset[0] alone
    BS_HIP(ctx, hipMemsetAsync(d_face_offset, 0, 4, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    return BS_OK;
  }
  DevBuf* B = ctx->ps;
  const In A{ctx->uc_xy, ctx->uc_z, ctx->uc_right, ctx->uc_ring, ctx->uc_soff, B[PS_RLABEL].as<int32_t>(), B[PS_LC].as<int32_t>(),
             B[PS_LV0].as<int32_t>(), B[PS_TB2].as<long long>(), B[PS_TOFF].as<long long>(), ctx->tr_tri, ctx->ps_nsv, ctx->ps_nr,
             ctx->ps_nl, 0, ctx->ps_base, ctx->ps_bin, ctx->ps_ntri,
             // (bs_set_building_bases ends the validity of a count, so the table is still the count's)
             ctx->ps_bases ? ctx->bases_dev.as<int32_t>() : nullptr, nullptr, 0};
  const Mesh o{reinterpret_cast<int4*>(d_vertex), d_face_offset, d_face_index, d_face_building, d_face_kind, nv, nf, ni};
  int* d_err = B[PS_MISC].as<int>() + W_ERR;
  const int32_t *vnum = B[PS_VNUM].as<int32_t>(), *wscan = B[PS_WSCAN].as<int32_t>();
  const long long* iscan = B[PS_ISCAN].as<long long>();
  Events<3> ev;
  for (int k = 0; k < 3; k++)
    BS_HIP(ctx, hipEventCreate(&ev.e[k]));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_err, 0, 4, st));
  ps_emit_vertex_kernel<<<sweep(nv), 256, 0, st>>>(A, B[PS_VSRC].as<int32_t>(), o, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  ps_emit_tri_kernel<<<sweep(A.ntri), 256, 0, st>>>(A, vnum, wscan, iscan, o, d_err);
  ps_emit_wall_kernel<<<sweep(A.nsv), 256, 0, st>>>(A, B[PS_TWIN].as<int32_t>(), vnum, B[PS_WCNT].as<int32_t>(), wscan, iscan, o, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  int h_err = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  if (h_err)
    return internal(ctx, h_err);
  ctx->ps_ms_emit[0] = ev.ms(0, 1);
  ctx->ps_ms_emit[1] = ev.ms(1, 2);
  return BS_OK;
}

extern "C" int bs_poly_solids(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height, int32_t n_labels,
                              int64_t num, int64_t den, int32_t cell_log2, const int32_t* label_building, int32_t n_buildings,
                              int32_t bin, int32_t base_z, struct bs_poly_solids* out, struct bs_outline_triangles* tri,
                              struct bs_clean_outlines* clean, struct bs_simple_outlines* simple, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->ps_valid = false;
  int rc = check_args(ctx, label, top, label_building, n_labels, n_buildings, bin, out);
  if (rc != BS_OK)
    return rc;
  Chain ch;
  rc = bs_outline_triangles(ctx, label, top, width, height, n_labels, num, den, cell_log2, &ch.tri, &ch.clean, &ch.simple, &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_tri = ch.has_clean = ch.has_simple = ch.has_plain = true;
  struct bs_poly_solids res;
  memset(&res, 0, sizeof res);
  ResultGuard guard{&res};
  DevBuf* B = ctx->ps;
  Staging S(ctx);
  // (without a label, label_building may be NULL: the slot then holds one entry that nobody reads, as it always has)
  const int32_t* d_lb = n_labels > 0 ? S.upload(B[PS_IN_LB], label_building, (size_t)n_labels) : S.room<int32_t>(B[PS_IN_LB], 1);
  if (!S.ok())
    return S.status();
  rc = poly_solids(ctx, ch.tri, ch.clean, width, d_lb, n_buildings, bin, base_z, res);
  if (rc != BS_OK)
    return rc;
  DevMesh mesh(res.n_vertices, res.n_faces, res.n_indices);
  mesh.place(S.room<char>(B[PS_OUT], mesh.bytes()));
  if (!S.ok())
    return S.status();
  ctx->ps_valid = true;
  rc = bs_poly_solids_emit_dev(ctx, mesh.vertex, mesh.face_offset, mesh.face_index, mesh.face_building, mesh.face_kind);
  ctx->ps_valid = false;
  if (rc != BS_OK)
    return rc;
  if (!mesh.to_host(S, res))
    return fail(ctx, BS_ERR_NOMEM, "polygon solids: host allocation");
  rc = S.finish();
  if (rc != BS_OK)
    return rc;
  res.ms_emit_vertices = ctx->ps_ms_emit[0];
  res.ms_emit_faces = ctx->ps_ms_emit[1];
  guard.keep = true;
  ch.hand_over(tri, clean, simple, plain);
  *out = res;
  ctx->ps_valid = true;
  return BS_OK;
}
