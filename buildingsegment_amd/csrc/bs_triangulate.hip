// bs_triangulate.hip -- every label's clean rings, holes included, as triangles over the clean vertices (DESIGN.md "Outline
// triangles"; the definition is written down in include/bs_api.h under "outline triangles").
//   clean     bs_clean_outlines_count_dev with max_rounds = -1 on the same images: the clean vertices, the ring of every
//             vertex and the first vertex of every ring stay on the device (bs_ctx::uc_xy, uc_ring, uc_soff)
//   prologue  the host holds every per-ring figure already: per label its rings, vertices V, holes H, outer rings O, its
//             occurrences V + 2 H, its first triangle (V + 2 H - 2 O each) and its bin; one upload, with the kernels'
//             arguments as one struct in device memory.  On the device the leftmost vertex of every hole, by two passes of
//             atomic minima over the vertices.
//   labels    one work item per label: the bridges in the order of the holes, then the ear scan list by list -- both
//             sequential chains; the lanes stride over the candidates and blockers of a bridge and over the blockers of an
//             ear test.  Three launches of one body: a wave per label with its slots in 1.25 KiB of LDS (up to
//             BS_TRI_WAVE_CAP occurrences), a workgroup of 256 with 20 KiB of LDS (up to BS_TRI_LDS_CAP), a workgroup of 256
//             with the same five arrays in a global workspace (beyond).
// A slot is an occurrence: slot i < V is vertex vbase + i of the label, slots V + 2 j and V + 2 j + 1 are the second
// occurrences M', V' of the j-th bridge.  Per slot five words: x, y, next, prev and the label-local vertex with two flags
// (in a list; in the current list and not yet clipped).  Every edge slot -> next[slot] of every slot in use is a ring
// segment or a bridge, so the blockers of a bridge are exactly those.
// The host reads once, for the result.  Every index read from memory is checked before it is used as an address; a
// violation sets err and the call returns BS_ERR_INTERNAL.
// The entry points own the results of the stages before and their own through bs_chain.h's Chain and hand them over at their
// end; an early return frees them.  Launch sizes, events and host arrays are bs_host.h's.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_chain.h"
#include "bs_common.h"
#include "bs_host.h"

namespace bs {
namespace {

// scratch of bs_ctx::tr
enum { TR_MISC, TR_ARGS, TR_DESC, TR_LIST, TR_OUTER, TR_RKEY, TR_RM, TR_LOUT, TR_BRIDGE, TR_TRI, TR_WS, TR_OUT, TR_TOFF, TR_COUNT };
static_assert(TR_COUNT <= (int)(sizeof(bs_ctx::tr) / sizeof(DevBuf)), "bs_ctx::tr is too short");

constexpr int32_t F_IN = 1 << 29, F_CUR = 1 << 30, IDX = F_IN - 1;
constexpr unsigned long long NONE = ~0ull;

struct LabelDesc {  // per label, from the host
  int32_t r0, r1;   // its rings
  int32_t vbase, V; // its vertices
  int32_t H, O;     // holes, outer rings
  long long tri_off;  // its first triangle
  long long ws_off;   // its first slot in the global workspace (the global path only)
};

struct LabelOut {  // per label, to the host
  long long area2, tests;
  int32_t status, pad;
};

struct TriArgs {  // in device memory: a kernel loads what it needs where it needs it
  const LabelDesc* desc;
  const int32_t* list;    // the labels by bin
  const int2* xy;         // the clean vertices
  const int32_t* ring;    // the ring of every vertex
  const int32_t* soff;    // the first vertex of every ring
  const uint8_t* outer;   // per ring
  const int32_t* ring_m;  // the leftmost vertex of every hole
  int32_t* tri;
  LabelOut* out;
  int2* bridge;
  int32_t* ws;         // the global workspace: 5 ws_total words, a label's five arrays side by side from 5 ws_off on
  long long ws_total;
  long long ntri;
  int32_t nr, nsv, n_labels, pad;
  int* err;
};

template <int CAP>
struct Store {  // a label's slots: five arrays of CAP words in LDS, or of the label's own occurrences n (5 n < 2^32) in its
  int32_t* b;   // part of the global workspace
  uint32_t n;
  __device__ uint32_t stride() const { return CAP > 0 ? (uint32_t)CAP : n; }
  __device__ int32_t& px(int32_t s) const { return b[(uint32_t)s]; }
  __device__ int32_t& py(int32_t s) const { return b[stride() + (uint32_t)s]; }
  __device__ int32_t& vt(int32_t s) const { return b[2u * stride() + (uint32_t)s]; }
  __device__ int32_t& nx(int32_t s) const { return b[3u * stride() + (uint32_t)s]; }
  __device__ int32_t& pv(int32_t s) const { return b[4u * stride() + (uint32_t)s]; }
};

struct Scratch {
  unsigned long long k0, k1;
  int32_t cnt;
};

__device__ inline unsigned long long lex(int x, int y) { return ((unsigned long long)(uint32_t)x << 32) | (uint32_t)y; }

// ---- prologue: the leftmost vertex of every hole, ties to the lower Y, then to the lower vertex ----
__global__ __launch_bounds__(256) void tri_ring_init_kernel(int32_t nr, unsigned long long* __restrict__ rkey, int32_t* __restrict__ rm)
{
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nr; r += (int64_t)gridDim.x * blockDim.x) {
    rkey[r] = NONE;
    rm[r] = INT_MAX;
  }
}

template <int PASS>
__global__ __launch_bounds__(256) void tri_ring_left_kernel(const int2* __restrict__ xy, const int32_t* __restrict__ ring,
                                                            const uint8_t* __restrict__ outer, int32_t nsv, int32_t nr,
                                                            unsigned long long* __restrict__ rkey, int32_t* __restrict__ rm,
                                                            int* __restrict__ err)
{
  for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < nsv; d += (int64_t)gridDim.x * blockDim.x) {
    const int32_t r = ring[d];
    if ((uint32_t)r >= (uint32_t)nr) {
      atomicOr(err, 1);
      continue;
    }
    if (outer[r])
      continue;
    const int2 p = xy[d];
    if (PASS == 0)
      atomicMin(rkey + r, lex(p.x, p.y));
    else if (rkey[r] == lex(p.x, p.y))
      atomicMin(rm + r, (int32_t)d);
  }
}

// ---- predicates ----
__device__ inline long long orient(int2 a, int2 b, int2 c)
{
  return (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
}

__device__ inline bool same(int2 a, int2 b) { return a.x == b.x && a.y == b.y; }

__device__ inline bool in_box(int2 a, int2 b, int2 p)
{
  return p.x >= min(a.x, b.x) && p.x <= max(a.x, b.x) && p.y >= min(a.y, b.y) && p.y <= max(a.y, b.y);
}

// the direction d in the cone at v between its predecessor p and its successor n
__device__ inline bool in_cone(int2 p, int2 v, int2 n, long long dx, long long dy)
{
  const long long nx = n.x - v.x, ny = n.y - v.y, qx = p.x - v.x, qy = p.y - v.y;
  if (orient(p, v, n) > 0)
    return nx * dy - ny * dx > 0 && dx * qy - dy * qx > 0;
  return !(qx * dy - qy * dx >= 0 && dx * ny - dy * nx >= 0);
}

__device__ inline bool blocks(int2 s, int2 e, int2 M, int2 V)
{
  if (max(s.x, e.x) < min(M.x, V.x) || max(M.x, V.x) < min(s.x, e.x) || max(s.y, e.y) < min(M.y, V.y) ||
      max(M.y, V.y) < min(s.y, e.y))
    return false;  // (closed segments whose boxes are apart have no common point)
  const long long o1 = orient(M, V, s), o2 = orient(M, V, e), o3 = orient(s, e, M), o4 = orient(s, e, V);
  if (((o1 > 0 && o2 < 0) || (o1 < 0 && o2 > 0)) && ((o3 > 0 && o4 < 0) || (o3 < 0 && o4 > 0)))
    return true;
  if (o1 == 0 && !same(s, M) && !same(s, V) && in_box(M, V, s))
    return true;
  if (o2 == 0 && !same(e, M) && !same(e, V) && in_box(M, V, e))
    return true;
  if (o3 == 0 && !same(M, s) && !same(M, e) && in_box(s, e, M))
    return true;
  return o4 == 0 && !same(V, s) && !same(V, e) && in_box(s, e, V);
}

// ---- one label ----
// Every thread of the group keeps the same control state, read from the shared arrays behind a barrier; thread 0 writes.
// (The strided passes are kept from unrolling: each is one short pass between two barriers of a chain of dependent steps.)
template <int NT, int CAP>
__device__ int tri_label(const int32_t l, const LabelDesc L, const Store<CAP> S, const TriArgs* __restrict__ G, Scratch* sh)
{
  const int tid = threadIdx.x;
  const int32_t V = L.V, nocc = L.V + 2 * L.H, vb = L.vbase;
  const int32_t ntri = nocc - 2 * L.O;
  auto pos = [&](int32_t s) { return make_int2(S.px(s), S.py(s)); };
  auto fail_label = [&](int32_t status) {  // no triangles, no bridges
    _Pragma("unroll 1") for (long long t = tid; t < 3ll * ntri; t += NT)
      G->tri[3 * L.tri_off + t] = -1;
    _Pragma("unroll 1") for (int32_t r = L.r0 + tid; r < L.r1; r += NT)
      G->bridge[r] = make_int2(-1, -1);
    if (tid == 0) {
      G->out[l].status = status;
      G->out[l].area2 = 0;
    }
  };
  // the rings as cyclic lists
  bool bad = false;
  _Pragma("unroll 1") for (int32_t s = tid; s < V; s += NT) {
    const int32_t r = G->ring[vb + s];
    int32_t a = 0, b = 0;
    if (r < L.r0 || r >= L.r1) {
      bad = true;
    } else {
      a = G->soff[r] - vb;
      b = G->soff[r + 1] - vb;
      bad |= a < 0 || a > s || b <= s || b > V || b - a < 3;
    }
    if (bad)
      a = s, b = s + 1;
    const int2 p = G->xy[vb + s];
    S.px(s) = p.x;
    S.py(s) = p.y;
    S.nx(s) = s + 1 < b ? s + 1 : a;
    S.pv(s) = s > a ? s - 1 : b - 1;
    S.vt(s) = s | (!bad && G->outer[r] ? F_IN : 0);
  }
  _Pragma("unroll 1") for (int32_t s = V + tid; s < nocc; s += NT) {
    S.px(s) = S.py(s) = S.vt(s) = 0;
    S.nx(s) = S.pv(s) = s;
  }
  _Pragma("unroll 1") for (int32_t r = L.r0 + tid; r < L.r1; r += NT)
    G->bridge[r] = make_int2(-1, -1);
  if (__syncthreads_or(bad)) {
    return 2;
  }
  // ---- bridges ----
  unsigned long long last_key = 0;
  int32_t last_m = -1;
  for (int32_t j = 0; j < L.H; j++) {
    // the next hole: the least (x, y, vertex) of a leftmost vertex behind the last one taken
    if (tid == 0)
      sh->k0 = sh->k1 = NONE;
    __syncthreads();
    _Pragma("unroll 1") for (int32_t r = L.r0 + tid; r < L.r1; r += NT) {
      if (G->outer[r])
        continue;
      const int32_t m = G->ring_m[r] - vb;
      if ((uint32_t)m >= (uint32_t)V) {
        bad = true;
        continue;
      }
      const unsigned long long key = lex(S.px(m), S.py(m));
      if (key > last_key || (key == last_key && m > last_m))
        atomicMin(&sh->k0, key);
    }
    __syncthreads();
    const unsigned long long key = sh->k0;
    _Pragma("unroll 1") for (int32_t r = L.r0 + tid; r < L.r1; r += NT) {
      if (G->outer[r])
        continue;
      const int32_t m = G->ring_m[r] - vb;
      if ((uint32_t)m < (uint32_t)V && lex(S.px(m), S.py(m)) == key && (key > last_key || m > last_m))
        atomicMin(&sh->k1, ((unsigned long long)(uint32_t)m << 32) | (uint32_t)(r - L.r0));
    }
    __syncthreads();
    const unsigned long long pick = sh->k1;
    if (__syncthreads_or(bad || pick == NONE)) {
      return 4;
    }
    const int32_t m = (int32_t)(pick >> 32), r = L.r0 + (int32_t)(pick & 0xFFFFFFFFu);
    last_key = key;
    last_m = m;
    const int32_t used = V + 2 * j;  // slots in use
    const int32_t mp = S.pv(m), mn = S.nx(m);
    if ((uint32_t)mp >= (uint32_t)V || (uint32_t)mn >= (uint32_t)V) {  // (uniform: every thread reads the same)
      return 4;
    }
    const int2 M = pos(m), Mp = pos(mp), Mn = pos(mn);
    // candidates by ascending (|V - M|^2, vertex, slot): the cones first, the blockers of the least one that is left
    unsigned long long lo_d2 = 0, lo_vs = 0;
    bool first = true;
    int32_t c = -1;
    for (int32_t round = 0; round <= used; round++) {
      if (tid == 0)
        sh->k0 = sh->k1 = NONE;
      __syncthreads();
      unsigned long long my_d2 = NONE, my_vs = NONE;
      _Pragma("unroll 1") for (int32_t s = tid; s < used; s += NT) {
        const int32_t w = S.vt(s);
        if (!(w & F_IN))
          continue;
        const int2 P = pos(s);
        if (same(P, M))
          continue;
        const long long dx = M.x - P.x, dy = M.y - P.y;
        const unsigned long long d2 = (unsigned long long)(dx * dx + dy * dy);
        const unsigned long long vs = ((unsigned long long)(uint32_t)(w & IDX) << 32) | (uint32_t)s;
        if (!first && (d2 < lo_d2 || (d2 == lo_d2 && vs <= lo_vs)))
          continue;
        if (d2 > my_d2 || (d2 == my_d2 && vs > my_vs))
          continue;
        const int32_t p = S.pv(s), n = S.nx(s);
        if ((uint32_t)p >= (uint32_t)used || (uint32_t)n >= (uint32_t)used) {
          bad = true;
          continue;
        }
        if (in_cone(pos(p), P, pos(n), dx, dy) && in_cone(Mp, M, Mn, -dx, -dy))
          my_d2 = d2, my_vs = vs;
      }
      if (my_d2 != NONE)
        atomicMin(&sh->k0, my_d2);
      __syncthreads();
      const unsigned long long d2 = sh->k0;
      if (my_d2 == d2 && d2 != NONE)
        atomicMin(&sh->k1, my_vs);
      __syncthreads();
      const unsigned long long vs = sh->k1;
      if (__syncthreads_or(bad)) {
        return 8;
      }
      if (d2 == NONE)
        break;  // no candidate is left
      const int32_t cs = (int32_t)(vs & 0xFFFFFFFFu);
      const int2 Vp = pos(cs);
      bool hit = false;
      _Pragma("unroll 1") for (int32_t s = tid; s < used && !hit; s += NT) {
        const int32_t e = S.nx(s);
        if ((uint32_t)e >= (uint32_t)used)
          bad = true;
        else
          hit = blocks(pos(s), pos(e), M, Vp);
      }
      if (!__syncthreads_or(hit)) {
        c = cs;
        break;
      }
      lo_d2 = d2;
      lo_vs = vs;
      first = false;
    }
    if (__syncthreads_or(bad)) {
      return 8;
    }
    if (c < 0) {
      fail_label(BS_TRI_NO_BRIDGE);
      return 0;
    }
    // ... V, M, (the hole from M round), M', V', ...
    const int32_t a = G->soff[r] - vb, b = G->soff[r + 1] - vb;
    if (a < 0 || a > m || b <= m || b > V) {
      return 8;
    }
    _Pragma("unroll 1") for (int32_t s = a + tid; s < b; s += NT)
      S.vt(s) |= F_IN;
    if (tid == 0) {
      const int32_t d0 = used, d1 = used + 1, on = S.nx(c), cv = S.vt(c) & IDX;
      S.nx(c) = m;
      S.pv(m) = c;
      S.nx(mp) = d0;
      S.pv(d0) = mp;
      S.nx(d0) = d1;
      S.pv(d1) = d0;
      S.nx(d1) = on;
      S.pv(on) = d1;
      S.px(d0) = M.x;
      S.py(d0) = M.y;
      S.vt(d0) = m | F_IN;
      S.px(d1) = S.px(c);
      S.py(d1) = S.py(c);
      S.vt(d1) = cv | F_IN;
      G->bridge[r] = make_int2(vb + m, vb + cv);
    }
    __syncthreads();
  }
  // ---- ears ----
  int32_t nt = 0;
  long long area = 0, tests = 0;
  for (int32_t r = L.r0; r < L.r1; r++) {
    if (!G->outer[r])
      continue;
    const int32_t start = G->soff[r] - vb;
    if ((uint32_t)start >= (uint32_t)V) {
      return 16;
    }
    if (tid == 0)
      sh->cnt = 0;
    __syncthreads();
    if (L.O == 1) {  // every slot in a list is in this one
      int32_t n = 0;
      _Pragma("unroll 1") for (int32_t s = tid; s < nocc; s += NT)
        if (S.vt(s) & F_IN) {
          S.vt(s) |= F_CUR;
          n++;
        }
      if (n)
        atomicAdd(&sh->cnt, n);
    } else if (tid == 0) {
      int32_t n = 0, s = start;
      do {
        S.vt(s) |= F_CUR;
        s = S.nx(s);
        n++;
      } while (s != start && (uint32_t)s < (uint32_t)nocc && n <= nocc);
      sh->cnt = s == start ? n : -1;
    }
    __syncthreads();
    int32_t left = sh->cnt;
    if (left < 3 || left > nocc) {
      return 16;
    }
    int32_t cur = start, stop = start, idle = 0;  // (idle: tests since the last ear; a list that is a cycle stalls in time)
    while (left > 3) {
      const int32_t b = cur, a = S.pv(b), c = S.nx(b);
      if ((uint32_t)a >= (uint32_t)nocc || (uint32_t)c >= (uint32_t)nocc || nt + 1 >= ntri || idle++ > nocc) {
        return 16;
      }
      const int2 A = pos(a), B = pos(b), C = pos(c);
      const long long o = orient(A, B, C);
      tests++;
      bool ear = false;
      if (o > 0) {
        bool hit = false;
        _Pragma("unroll 1") for (int32_t s = tid; s < nocc && !hit; s += NT) {
          if (!(S.vt(s) & F_CUR))
            continue;
          const int2 Q = pos(s);
          hit = !same(Q, A) && !same(Q, B) && !same(Q, C) && orient(A, B, Q) >= 0 && orient(B, C, Q) >= 0 && orient(C, A, Q) >= 0;
        }
        ear = !__syncthreads_or(hit);
      }
      if (ear) {
        if (tid == 0) {
          int32_t* t = G->tri + 3 * (L.tri_off + nt);
          t[0] = vb + (S.vt(a) & IDX);
          t[1] = vb + (S.vt(b) & IDX);
          t[2] = vb + (S.vt(c) & IDX);
          S.nx(a) = c;
          S.pv(c) = a;
          S.vt(b) &= ~F_CUR;
        }
        nt++;
        area += o;
        left--;
        idle = 0;
        __syncthreads();
        cur = stop = S.nx(c);
        if ((uint32_t)cur >= (uint32_t)nocc) {
          return 16;
        }
      } else {
        cur = c;
        if (cur == stop) {
          if (tid == 0)
            G->out[l].tests = tests;
          fail_label(BS_TRI_STALLED);
          return 0;
        }
      }
    }
    const int32_t a = S.pv(cur), c = S.nx(cur);
    if ((uint32_t)a >= (uint32_t)nocc || (uint32_t)c >= (uint32_t)nocc || nt >= ntri) {
      return 16;
    }
    area += orient(pos(a), pos(cur), pos(c));
    if (tid == 0) {
      int32_t* t = G->tri + 3 * (L.tri_off + nt);
      t[0] = vb + (S.vt(a) & IDX);
      t[1] = vb + (S.vt(cur) & IDX);
      t[2] = vb + (S.vt(c) & IDX);
      S.vt(a) &= ~F_CUR;
      S.vt(cur) &= ~F_CUR;
      S.vt(c) &= ~F_CUR;
    }
    nt++;
    __syncthreads();
  }
  if (nt != ntri) {
    return 32;
  }
  if (tid == 0)
    G->out[l] = LabelOut{area, tests, BS_TRI_OK, 0};
  return 0;
}

// One workgroup per label of the bin [first, first + n) of the list.  CAP > 0: the slots in LDS, a label of more
// occurrences is an error; CAP = 0: in the workspace.  Returns of tri_label other than 0 are phase masks of the error word.
template <int NT, int CAP>
__global__ __launch_bounds__(NT) void tri_labels_kernel(const TriArgs* __restrict__ A, int32_t first)
{
  __shared__ int32_t lds[CAP > 0 ? 5 * CAP : 1];
  __shared__ Scratch sh;
  const int32_t l = A->list[first + blockIdx.x];
  int code = 64;
  if ((uint32_t)l < (uint32_t)A->n_labels) {
    const LabelDesc L = A->desc[l];
    const long long nocc = (long long)L.V + 2ll * L.H, ntri = nocc - 2ll * L.O;
    bool ok = L.r0 >= 0 && L.r0 < L.r1 && L.r1 <= A->nr && L.vbase >= 0 && L.V >= 3 && (long long)L.vbase + L.V <= A->nsv &&
              L.H >= 0 && L.O >= 0 && L.H + L.O == L.r1 - L.r0 && nocc < F_IN && ntri >= 0 && L.tri_off >= 0 &&
              L.tri_off + ntri <= A->ntri;
    Store<CAP> S;
    if (CAP > 0) {
      ok = ok && nocc <= CAP;
      S = Store<CAP>{lds, (uint32_t)CAP};
    } else {
      ok = ok && L.ws_off >= 0 && L.ws_off + nocc <= A->ws_total;
      S = Store<CAP>{A->ws + (ok ? 5 * L.ws_off : 0), (uint32_t)nocc};
    }
    if (ok)
      code = tri_label<NT, CAP>(l, L, S, A, &sh);
  }
  if (code && threadIdx.x == 0)
    atomicOr(A->err, code);
}

__global__ __launch_bounds__(256) void tri_emit_kernel(const int32_t* __restrict__ src, int64_t n, int32_t* __restrict__ dst)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

int internal(bs_ctx* ctx, int err)
{
  char msg[96];
  snprintf(msg, sizeof msg, "outline triangles: an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

// the triangles of the clean outlines c, whose count has just run on ctx; res is zeroed
int triangulate(bs_ctx* ctx, const struct bs_clean_outlines& c, struct bs_outline_triangles& res)
{
  const int32_t nl = c.n_labels;
  const int64_t nr64 = c.n_rings, nsv64 = c.n_svertices;
  if (nsv64 >= (1ll << 31) || nr64 >= (1ll << 31))
    return fail(ctx, BS_ERR_INVALID, "outline triangles: 2^31 clean vertices or more");
  const int32_t nr = (int32_t)nr64, nsv = (int32_t)nsv64;
  res.n_labels = nl;
  res.wave_cap = BS_TRI_WAVE_CAP;
  res.lds_cap = BS_TRI_LDS_CAP;
  res.n_rings = nr;
  res.n_svertices = nsv;
  res.ms_clean = c.ms_simplify + c.ms_detect + c.ms_repair + c.ms_rings;
  const bool ok[] = {alloc(&res.tri_offset, (size_t)nl + 1), alloc(&res.label_status, (size_t)nl), alloc(&res.label_area2, (size_t)nl),
                     alloc(&res.label_tests, (size_t)nl), alloc(&res.bridge, 2 * (size_t)nr)};
  if (!std::all_of(std::begin(ok), std::end(ok), [](bool b) { return b; }))
    return fail(ctx, BS_ERR_NOMEM, "outline triangles: host allocation");
  // ---- prologue on the host: every per-ring figure is here already ----
  std::vector<LabelDesc> desc((size_t)std::max(nl, 1));
  std::vector<int32_t> bins[3];
  std::vector<uint8_t> outer((size_t)std::max(nr, 1));
  for (int32_t r = 0; r < nr; r++)
    outer[r] = c.ring_area2[r] > 0;
  long long ntri = 0, ws_total = 0;
  for (int32_t l = 0; l < nl; l++) {
    const int64_t r0 = c.label_ring_offset[l], r1 = c.label_ring_offset[l + 1];
    if (r0 < 0 || r0 > r1 || r1 > nr)
      return internal(ctx, 0x10000);
    LabelDesc& L = desc[l];
    L = LabelDesc{(int32_t)r0, (int32_t)r1, (int32_t)c.s_ring_offset[r0], (int32_t)(c.s_ring_offset[r1] - c.s_ring_offset[r0]), 0, 0, ntri, 0};
    for (int64_t r = r0; r < r1; r++)
      (outer[r] ? L.O : L.H)++;
    const long long nocc = (long long)L.V + 2ll * L.H;
    if (nocc >= F_IN)
      return fail(ctx, BS_ERR_INVALID, "outline triangles: a label of 2^29 occurrences or more");
    res.tri_offset[l] = ntri;
    res.label_status[l] = BS_TRI_EMPTY;
    if (r0 == r1)
      continue;
    ntri += nocc - 2ll * L.O;
    res.max_label_occurrences = std::max<int64_t>(res.max_label_occurrences, nocc);
    const int bin = nocc <= BS_TRI_WAVE_CAP ? 0 : nocc <= BS_TRI_LDS_CAP ? 1 : 2;
    bins[bin].push_back(l);
    if (bin == 2) {
      L.ws_off = ws_total;
      ws_total += nocc;
    }
  }
  res.tri_offset[nl] = ntri;
  res.n_triangles = ntri;
  res.n_labels_wave = (int64_t)bins[0].size();
  res.n_labels_lds = (int64_t)bins[1].size();
  res.n_labels_global = (int64_t)bins[2].size();
  if (3 * ntri >= (1ll << 40))
    return fail(ctx, BS_ERR_INVALID, "outline triangles: too many triangles");
  for (int64_t r = 0; r < 2 * (int64_t)nr; r++)
    res.bridge[r] = -1;
  ctx->tr_ntri = ntri;
  ctx->tr_tri = nullptr;
  ctx->tr_toff = nullptr;  // (for bs_modelraster.hip)
  ctx->tr_nl = nl;
  ctx->tr_w = c.width;
  ctx->tr_h = c.height;
  if (nr == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->tr;
  Events<5> ev;
  for (int i = 0; i < 5; i++)
    BS_HIP(ctx, hipEventCreate(&ev.e[i]));
  std::vector<int32_t> list;
  for (auto& b : bins)
    list.insert(list.end(), b.begin(), b.end());
  BS_HIP(ctx, B[TR_MISC].reserve(256));
  BS_HIP(ctx, B[TR_DESC].reserve(sizeof(LabelDesc) * (size_t)std::max(nl, 1)));
  BS_HIP(ctx, B[TR_LIST].reserve(4 * list.size()));
  BS_HIP(ctx, B[TR_OUTER].reserve((size_t)nr));
  BS_HIP(ctx, B[TR_RKEY].reserve(8 * (size_t)nr));
  BS_HIP(ctx, B[TR_RM].reserve(4 * (size_t)nr));
  BS_HIP(ctx, B[TR_ARGS].reserve(sizeof(TriArgs)));
  BS_HIP(ctx, B[TR_LOUT].reserve(sizeof(LabelOut) * (size_t)nl));
  BS_HIP(ctx, B[TR_BRIDGE].reserve(8 * (size_t)nr));
  BS_HIP(ctx, B[TR_TRI].reserve(12 * (size_t)std::max<long long>(ntri, 1)));
  BS_HIP(ctx, B[TR_WS].reserve(20 * (size_t)std::max<long long>(ws_total, 1)));
  BS_HIP(ctx, B[TR_TOFF].reserve(8 * ((size_t)nl + 1)));
  int* d_err = B[TR_MISC].as<int>();
  uint8_t* d_outer = B[TR_OUTER].as<uint8_t>();
  unsigned long long* rkey = B[TR_RKEY].as<unsigned long long>();
  int32_t* rm = B[TR_RM].as<int32_t>();
  ctx->tr_tri = B[TR_TRI].as<int32_t>();  // (for bs_polysolid.hip)
  const TriArgs args{B[TR_DESC].as<LabelDesc>(), B[TR_LIST].as<int32_t>(), ctx->uc_xy, ctx->uc_ring, ctx->uc_soff, d_outer, rm,
                     B[TR_TRI].as<int32_t>(), B[TR_LOUT].as<LabelOut>(), B[TR_BRIDGE].as<int2>(), B[TR_WS].as<int32_t>(), ws_total,
                     ntri, nr, nsv, nl, 0, d_err};
  const TriArgs* d_args = B[TR_ARGS].as<TriArgs>();
  if (!args.xy || !args.ring || !args.soff)
    return internal(ctx, 0x20000);
  std::vector<LabelOut> lout((size_t)nl, LabelOut{0, 0, BS_TRI_EMPTY, 0});
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  BS_HIP(ctx, hipMemsetAsync(d_err, 0, 4, st));
  BS_HIP(ctx, hipMemcpyAsync(B[TR_ARGS].p, &args, sizeof args, hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[TR_DESC].p, desc.data(), sizeof(LabelDesc) * (size_t)nl, hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[TR_LIST].p, list.data(), 4 * list.size(), hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(d_outer, outer.data(), (size_t)nr, hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[TR_LOUT].p, lout.data(), sizeof(LabelOut) * (size_t)nl, hipMemcpyHostToDevice, st));
  BS_HIP(ctx, hipMemcpyAsync(B[TR_TOFF].p, res.tri_offset, 8 * ((size_t)nl + 1), hipMemcpyHostToDevice, st));
  ctx->tr_toff = B[TR_TOFF].as<long long>();
  tri_ring_init_kernel<<<sweep(nr), 256, 0, st>>>(nr, rkey, rm);
  tri_ring_left_kernel<0><<<sweep(nsv), 256, 0, st>>>(args.xy, args.ring, d_outer, nsv, nr, rkey, rm, d_err);
  tri_ring_left_kernel<1><<<sweep(nsv), 256, 0, st>>>(args.xy, args.ring, d_outer, nsv, nr, rkey, rm, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  const int32_t n0 = (int32_t)bins[0].size(), n1 = (int32_t)bins[1].size(), n2 = (int32_t)bins[2].size();
  if (n0 > 0)
    tri_labels_kernel<64, BS_TRI_WAVE_CAP><<<n0, 64, 0, st>>>(d_args, 0);
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  if (n1 > 0)
    tri_labels_kernel<256, BS_TRI_LDS_CAP><<<n1, 256, 0, st>>>(d_args, n0);
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  if (n2 > 0)
    tri_labels_kernel<256, 0><<<n2, 256, 0, st>>>(d_args, n0 + n1);
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  int h_err = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(lout.data(), B[TR_LOUT].p, sizeof(LabelOut) * (size_t)nl, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.bridge, B[TR_BRIDGE].p, 8 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the result
  BS_HIP(ctx, hipGetLastError());
  if (h_err)
    return internal(ctx, h_err);
  for (int32_t l = 0; l < nl; l++) {
    res.label_status[l] = lout[l].status;
    res.label_area2[l] = lout[l].area2;
    res.label_tests[l] = lout[l].tests;
  }
  for (int32_t l = 0; l < nl; l++) {
    const int32_t s = res.label_status[l];
    if (s < BS_TRI_OK || s > BS_TRI_EMPTY)
      return internal(ctx, 0x40000);
    res.n_failed_labels += s == BS_TRI_NO_BRIDGE || s == BS_TRI_STALLED;
    res.n_tests += res.label_tests[l];
  }
  for (int32_t r = 0; r < nr; r++)
    res.n_bridges += res.bridge[2 * r] >= 0;
  res.ms_prologue = ev.ms(0, 1);
  res.ms_wave = ev.ms(1, 2);
  res.ms_lds = ev.ms(2, 3);
  res.ms_global = ev.ms(3, 4);
  return BS_OK;
}

}  // namespace
}  // namespace bs

using namespace bs;

extern "C" void bs_outline_triangles_free(struct bs_outline_triangles* t)
{
  if (!t)
    return;
  free(t->tri_offset);
  free(t->label_status);
  free(t->label_area2);
  free(t->label_tests);
  free(t->bridge);
  free(t->tri);
  memset(t, 0, sizeof *t);
}

extern "C" int bs_outline_triangles_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width, int32_t height,
                                              int32_t n_labels, int64_t num, int64_t den, int32_t cell_log2,
                                              struct bs_outline_triangles* out, struct bs_clean_outlines* clean,
                                              struct bs_simple_outlines* simple, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->tr_valid = false;
  if (!out)
    return fail(ctx, BS_ERR_INVALID, "outline triangles: null pointer");
  Chain ch;  // (its triangles are this call's own result)
  int rc = bs_clean_outlines_count_dev(ctx, d_label, d_top, width, height, n_labels, num, den, -1, cell_log2, &ch.clean, &ch.simple,
                                       &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_plain = ch.has_simple = ch.has_clean = ch.has_tri = true;
  rc = triangulate(ctx, ch.clean, ch.tri);
  if (rc != BS_OK)
    return rc;
  ch.hand_over(out, clean, simple, plain);
  ctx->tr_valid = true;
  return BS_OK;
}

extern "C" int bs_outline_triangles_emit_dev(bs_ctx* ctx, int32_t* d_tri)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!ctx->tr_valid)
    return fail(ctx, BS_ERR_INVALID, "outline triangles: emit without a successful count on this context");
  const int64_t n = 3 * ctx->tr_ntri;
  if (n > 0 && !d_tri)
    return fail(ctx, BS_ERR_INVALID, "outline triangles: emit needs d_tri");
  ctx->tr_ms_emit = 0;
  if (n == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Events<2> ev;
  BS_HIP(ctx, hipEventCreate(&ev.e[0]));
  BS_HIP(ctx, hipEventCreate(&ev.e[1]));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  tri_emit_kernel<<<sweep(n), 256, 0, st>>>(ctx->tr[TR_TRI].as<int32_t>(), n, d_tri);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  ctx->tr_ms_emit = ev.ms(0, 1);
  return BS_OK;
}

extern "C" int bs_outline_triangles(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height,
                                    int32_t n_labels, int64_t num, int64_t den, int32_t cell_log2, struct bs_outline_triangles* out,
                                    struct bs_clean_outlines* clean, struct bs_simple_outlines* simple, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->tr_valid = false;
  if (!out)
    return fail(ctx, BS_ERR_INVALID, "outline triangles: null pointer");
  Chain ch;  // (its triangles are this call's own result)
  struct bs_outline_triangles& res = ch.tri;
  int rc = bs_clean_outlines(ctx, label, top, width, height, n_labels, num, den, -1, cell_log2, &ch.clean, &ch.simple, &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_plain = ch.has_simple = ch.has_clean = ch.has_tri = true;
  rc = triangulate(ctx, ch.clean, res);
  if (rc != BS_OK)
    return rc;
  const size_t n = 3 * (size_t)res.n_triangles;
  if (!alloc(&res.tri, n))
    return fail(ctx, BS_ERR_NOMEM, "outline triangles: host allocation");
  if (n > 0) {  // (the inputs went up in bs_clean_outlines: only the triangles are staged here)
    Staging S(ctx);
    int32_t* d_tri = S.room<int32_t>(ctx->tr[TR_OUT], n);
    if (!S.ok())
      return S.status();
    ctx->tr_valid = true;
    rc = bs_outline_triangles_emit_dev(ctx, d_tri);
    ctx->tr_valid = false;
    if (rc != BS_OK)
      return rc;
    S.download(res.tri, d_tri, n);
    rc = S.finish();
    if (rc != BS_OK)
      return rc;
    res.ms_emit = ctx->tr_ms_emit;
  }
  ch.hand_over(out, clean, simple, plain);
  ctx->tr_valid = true;
  return BS_OK;
}

extern "C" int bs_outline_triangles_write_obj(const struct bs_outline_triangles* t, const struct bs_clean_outlines* c, int32_t bin,
                                              const int32_t* origin, const char* path)
{
  if (!t || !c || !path || bin < 1 || t->n_labels < 0 || t->n_triangles < 0 || c->n_svertices < 0 || c->n_svertices != t->n_svertices)
    return BS_ERR_INVALID;
  if (!t->tri_offset || (t->n_labels > 0 && !t->label_status) || (t->n_triangles > 0 && !t->tri) || (c->n_svertices > 0 && !c->sxy))
    return BS_ERR_INVALID;
  if (t->tri_offset[0] != 0 || t->tri_offset[t->n_labels] != t->n_triangles)
    return BS_ERR_INVALID;
  for (int32_t l = 0; l < t->n_labels; l++) {
    if (t->tri_offset[l + 1] < t->tri_offset[l])
      return BS_ERR_INVALID;
    if (t->label_status[l] != BS_TRI_OK)
      continue;
    for (int64_t i = 3 * t->tri_offset[l]; i < 3 * t->tri_offset[l + 1]; i++)
      if (t->tri[i] < 0 || t->tri[i] >= c->n_svertices)
        return BS_ERR_INVALID;
  }
  FILE* fo = fopen(path, "w");
  if (!fo)
    return BS_ERR_INVALID;
  const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  fprintf(fo, "# outline triangles: %d labels, %lld vertices, %lld triangles, %lld failed labels, %lld bridges\n", t->n_labels,
          (long long)c->n_svertices, (long long)t->n_triangles, (long long)t->n_failed_labels, (long long)t->n_bridges);
  for (int64_t v = 0; v < c->n_svertices; v++)
    fprintf(fo, "v %lld %lld %lld\n", (long long)((int64_t)c->sxy[2 * v] * bin + org[0]),
            (long long)((int64_t)c->sxy[2 * v + 1] * bin + org[1]), (long long)((c->sz ? (int64_t)c->sz[v] : 0) + org[2]));
  for (int32_t l = 0; l < t->n_labels; l++) {
    if (t->label_status[l] != BS_TRI_OK)
      continue;
    fprintf(fo, "g label_%d\n", l);
    for (int64_t i = t->tri_offset[l]; i < t->tri_offset[l + 1]; i++)
      fprintf(fo, "f %d %d %d\n", t->tri[3 * i] + 1, t->tri[3 * i + 1] + 1, t->tri[3 * i + 2] + 1);
  }
  const bool ok = !ferror(fo);
  return (fclose(fo) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}
