// bs_simplify.hip -- the facet outlines simplified arc by arc with an exact Douglas-Peucker (DESIGN.md "Simplified
// outlines"; the definition is written down in include/bs_api.h under "simplified outlines").
//   outlines  bs_facet_outlines_count_dev on the same images: half-edges, successors, vertex flags, leaders, rings
//   nodes     per compact half-edge the junction test of its start corner (four label reads), node flag, right label,
//             corner index and Z
//   placing   the cut and the R Wyllie rounds of the outlines once more, carrying node counts: a node stands at (nodes of
//             its ring) - (its suffix count) in walk order from h0; the node counts scanned = the ring's first node
//   arcs      per ring the junction nodes, the first of them and the lowest (corner, place), reduced over runs of equal ring
//             inside a wave before one set of atomics per run; the rotation; every node scattered to its place in the
//             rotated order, so that a ring begins with an arc start and an arc is a run of the node arrays; arc ids from one
//             scan; the segment (left kept node, right kept node) of every node = its arc; the closed pass that keeps F
//   rounds    three kernels per round: the measure c^2 of every active node and its maximum per segment; the lowest
//             (corner << 32 | place) among the nodes that reach the maximum; the decision per node -- kept, dropped with its
//             whole segment, or one of the two new segments -- into the other buffer.  A segment is named by the kept node
//             at its left end, so no round searches for the nearest kept node: every node carries its two.
//   rings     the kept flags scanned; a kept node's place in its ring from the scan and the rotation; area2 over runs
//   emit      copies of the finished vertex arrays
// No thread walks a ring or an arc: the only loops in kernels are grid strides, the four pixels of a block and the steps of
// a wave scan.  Every index read from memory is checked before it is used as an address; a violation sets err and the call
// returns BS_ERR_INTERNAL.  No kernel reads an array that a thread of the same launch writes.
// The entry points own the plain outlines and their own result through bs_chain.h's Chain and hand them over at their end;
// an early return frees them.  bs_outline.h is what this file shares with bs_outline.hip (the ranking kernels, the scratch
// of bs_ctx::ol); launch sizes, events and host arrays are bs_host.h's.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bs_chain.h"
#include "bs_common.h"
#include "bs_outline.h"
#include "bs_segscan.h"

namespace bs {
namespace {

// scratch of bs_ctx::sp
enum { SP_MISC, SP_TMP, SP_HFLAG, SP_HRIGHT, SP_HCIDX, SP_HZ, SP_NX0, SP_NX1, SP_VAL0, SP_VAL1, SP_RING, SP_NXY, SP_NCIDX, SP_NZ,
       SP_NRIGHT, SP_NFLAG, SP_NRING, SP_ARC, SP_ASTART, SP_SEG0, SP_SEG1, SP_C2, SP_BEST0, SP_BEST1, SP_TIE0, SP_TIE1, SP_FORCED,
       SP_KSCAN, SP_FXY, SP_FZ, SP_FRIGHT, SP_FFLAG, SP_FRING, SP_IN_LABEL, SP_IN_TOP, SP_OUT_XY, SP_OUT_Z, SP_OUT_RIGHT,
       SP_OUT_FLAG, SP_COUNT };
static_assert(SP_COUNT <= (int)(sizeof(bs_ctx::sp) / sizeof(DevBuf)), "bs_ctx::sp is too short");

constexpr int NODE_GRID_CAP = 1024;  // workgroups of the grid-stride passes over half-edges and nodes: four per CU
constexpr int ROUND_BATCH = 4;  // rounds between two reads of the "kept something" words
constexpr int32_t KEPT = -1, DROPPED = -2;  // seg.x of a node that is no longer active
// words of SP_MISC
enum { W_ERR, W_MAXARC, W_CHANGED /* [ROUND_BATCH] */, W_COUNT = W_CHANGED + ROUND_BATCH };
// bits of hflag (per half-edge) and nflag (per node)
constexpr unsigned H_NODE = 1, H_JUNCTION = 2;
constexpr unsigned N_JUNCTION = 1, N_LONE_START = 2, N_ARC_START = 4;

struct RingFig {  // per ring in the listed order, device
  unsigned long long* lowest;  // (corner << 32) | place of the node with the lowest corner index
  unsigned long long* area2;   // of the kept nodes (two's complement sum)
  int32_t* nodes;
  int32_t* junctions;
  int32_t* first_junction;  // place of the first junction node in walk order from h0
  int32_t* rot;             // place of the node the rotated order begins with
  int32_t* noff;            // [n_rings + 1]: the ring's first node in the node arrays
  int32_t* soff;            // [n_rings + 1]: the ring's first kept vertex
};
constexpr size_t RING_FIG_BYTES = 2 * 8 + 6 * 4;  // (+ 8 for the two last offsets)

inline int node_grid(int64_t n) { return (int)std::min<int64_t>(nblk(n, 256), NODE_GRID_CAP); }

RingFig ring_fig_at(void* p, size_t n)
{
  RingFig f;
  f.lowest = (unsigned long long*)p;
  f.area2 = f.lowest + n;
  f.nodes = (int32_t*)(f.area2 + n);
  f.junctions = f.nodes + n;
  f.first_junction = f.junctions + n;
  f.rot = f.first_junction + n;
  f.noff = f.rot + n;
  f.soff = f.noff + n + 1;
  return f;
}

// ---- nodes ---------------------------------------------------------------------------------------------------------------
// Per compact half-edge: the block of its start corner (X, Y) is a = (X-1, Y-1), b = (X, Y-1), c = (X-1, Y), d = (X, Y),
// outside the image or negative = -1.  A junction: three or more distinct labels, or the saddle a b / b a.  The pixel across
// side k is one of the four: b, d, c, a for k = 0 .. 3.
__global__ __launch_bounds__(256) void simplify_nodes_kernel(const int32_t* __restrict__ label, const int32_t* __restrict__ top,
                                                             const int32_t* __restrict__ hnum, const uint8_t* __restrict__ vert,
                                                             int w, int h, int32_t n, uint8_t* __restrict__ hflag,
                                                             uint8_t* __restrict__ isnode,
                                                             int32_t* __restrict__ hright, int32_t* __restrict__ hcidx,
                                                             int32_t* __restrict__ hz, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const int32_t hn = hnum[i];
  const int64_t p = hn >> 2, npix = (int64_t)w * h;
  if (hn < 0 || p >= npix) {
    atomicOr(err, 1);
    hflag[i] = isnode[i] = 0;
    return;
  }
  const int k = hn & 3;
  const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
  const int X = x + (k == 1 || k == 2), Y = y + (k >= 2);
  int32_t b4[4];
  for (int j = 0; j < 4; j++) {
    const int px = X - 1 + (j & 1), py = Y - 1 + (j >> 1);
    int32_t l = -1;
    if (px >= 0 && px < w && py >= 0 && py < h)
      l = max(label[(int64_t)py * w + px], -1);
    b4[j] = l;
  }
  const int32_t a = b4[0], b = b4[1], c = b4[2], d = b4[3];
  const int distinct = 1 + (b != a) + (c != a && c != b) + (d != a && d != b && d != c);
  const bool junction = distinct >= 3 || (a == d && b == c && a != b);
  const bool node = vert[i] || junction;
  hflag[i] = (uint8_t)((node ? H_NODE : 0u) | (junction ? H_JUNCTION : 0u));
  isnode[i] = node;  // (the value the ranking carries)
  hright[i] = k == 0 ? b : k == 1 ? d : k == 2 ? c : a;
  hcidx[i] = Y * (w + 1) + X;
  if (top && node)
    hz[i] = top[4 * p + (k ^ (k >> 1))];  // the start corner of side k: t00, t10, t11, t01
}

// ---- placing ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void simplify_ring_init_kernel(RingFig F, int32_t nr)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nr)
    return;
  F.lowest[r] = ~0ull;
  F.area2[r] = 0;
  F.nodes[r] = F.junctions[r] = 0;
  F.first_junction[r] = INT32_MAX;
}

// the ring of half-edge i in the listed order, or -1
__device__ inline int32_t ring_of(const int32_t* __restrict__ leader, const int32_t* __restrict__ slot,
                                  const int32_t* __restrict__ of_slot, int64_t i, int32_t n, int32_t nr)
{
  const int32_t L = leader[i];
  const int32_t s = (uint32_t)L < (uint32_t)n ? slot[L] : -1;
  const int32_t r = (uint32_t)s < (uint32_t)nr ? of_slot[s] : -1;
  return (uint32_t)r < (uint32_t)nr ? r : -1;
}

// the suffix count of a leader is the node count of its ring
__global__ __launch_bounds__(256) void simplify_ring_nodes_kernel(const int32_t* __restrict__ leader, const int32_t* __restrict__ slot,
                                                                  const int32_t* __restrict__ of_slot, const int32_t* __restrict__ val,
                                                                  const int32_t* __restrict__ nxt, int32_t n, int32_t nr,
                                                                  int32_t* __restrict__ nodes, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  if (nxt[i] != END)
    atomicOr(err, 2);  // the list did not close within the rounds
  if (leader[i] != (int32_t)i)
    return;
  const int32_t r = ring_of(leader, slot, of_slot, i, n, nr);
  if (r < 0)
    atomicOr(err, 2);
  else
    nodes[r] = val[i];
}

struct NodeCount {  // the node count of ring r, 0 for the entry behind the last
  const int32_t* nodes;
  int32_t nr;
  __host__ __device__ int32_t operator()(int32_t r) const { return r < nr ? nodes[r] : 0; }
};

// ---- arcs ------------------------------------------------------------------------------------------------------------------
// One lane per half-edge; the figures of the nodes are reduced over the runs of equal ring inside the wave.
__global__ __launch_bounds__(256) void simplify_ring_figures_kernel(const uint8_t* __restrict__ hflag, const int32_t* __restrict__ hcidx,
                                                                    const int32_t* __restrict__ leader, const int32_t* __restrict__ slot,
                                                                    const int32_t* __restrict__ of_slot, const int32_t* __restrict__ val,
                                                                    const int32_t* __restrict__ nodes, int32_t n, int32_t nr,
                                                                    int32_t* __restrict__ junctions, int32_t* __restrict__ first_junction,
                                                                    unsigned long long* __restrict__ lowest, int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int64_t n64 = ((int64_t)n + 63) & ~(int64_t)63;  // whole waves stay together
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n64; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t r = -1, jc = 0, fj = INT32_MAX;
    unsigned long long low = ~0ull;
    if (i < n && (hflag[i] & H_NODE)) {
      r = ring_of(leader, slot, of_slot, i, n, nr);
      const int32_t nn = r >= 0 ? nodes[r] : 0, pos = nn - val[i];
      if (r < 0 || pos < 0 || pos >= nn) {
        atomicOr(err, 4);
        r = -1;
      } else {
        if (hflag[i] & H_JUNCTION)
          jc = 1, fj = pos;
        low = ((unsigned long long)(uint32_t)hcidx[i] << 32) | (uint32_t)pos;
      }
    }
    const int32_t prev = __shfl_up(r, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != r);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    BS_SEG_SCAN(jc, BS_OP_ADD)
    BS_SEG_SCAN(fj, BS_OP_MIN)
    BS_SEG_SCAN(low, BS_OP_MIN)
    if (lane == tl && r >= 0) {
      if (jc > 0) {
        atomicAdd(junctions + r, jc);
        atomicMin(first_junction + r, fj);
      }
      atomicMin(lowest + r, low);
    }
  }
}

// a ring begins, in the rotated order, with its first junction node, or without one with the node of its lowest corner
__global__ __launch_bounds__(256) void simplify_rot_kernel(RingFig F, int32_t nr, int* __restrict__ err)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r >= nr)
    return;
  int32_t rot = F.junctions[r] > 0 ? F.first_junction[r] : (int32_t)(F.lowest[r] & 0xFFFFFFFFull);
  if (rot < 0 || rot >= F.nodes[r]) {
    atomicOr(err, 8);
    rot = 0;
  }
  F.rot[r] = rot;
}

struct NodeArrays {  // per node in the rotated order, device
  int2* xy;
  int32_t* cidx;
  int32_t* z;
  int32_t* right;
  int32_t* ring;
  uint8_t* flag;
};

__global__ __launch_bounds__(256) void simplify_scatter_kernel(const uint8_t* __restrict__ hflag, const int32_t* __restrict__ hcidx,
                                                               const int32_t* __restrict__ hright, const int32_t* __restrict__ hz,
                                                               const int32_t* __restrict__ leader, const int32_t* __restrict__ slot,
                                                               const int32_t* __restrict__ of_slot, const int32_t* __restrict__ val,
                                                               RingFig F, int w, int32_t n, int32_t nr, int32_t N, bool has_z,
                                                               NodeArrays A, int* __restrict__ err)
{
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n)
    return;
  const unsigned f = hflag[i];
  if (!(f & H_NODE))
    return;
  const int32_t r = ring_of(leader, slot, of_slot, i, n, nr);
  if (r < 0) {
    atomicOr(err, 16);
    return;
  }
  const int32_t nn = F.nodes[r], pos = nn - val[i];
  int32_t q = pos - F.rot[r];
  if (q < 0)
    q += nn;
  const int64_t Q = (int64_t)F.noff[r] + q;
  if (pos < 0 || pos >= nn || q < 0 || q >= nn || Q < 0 || Q >= N) {
    atomicOr(err, 16);
    return;
  }
  const bool junction = f & H_JUNCTION, lone = q == 0 && F.junctions[r] == 0;
  const int32_t ci = hcidx[i];
  A.xy[Q] = make_int2(ci % (w + 1), ci / (w + 1));
  A.cidx[Q] = ci;
  A.right[Q] = hright[i];
  A.ring[Q] = r;
  A.flag[Q] = (uint8_t)((junction ? N_JUNCTION : 0u) | (lone ? N_LONE_START : 0u) | ((junction || q == 0) ? N_ARC_START : 0u));
  if (has_z)
    A.z[Q] = hz[i];
}

struct ArcStart {
  const uint8_t* flag;
  __host__ __device__ int32_t operator()(int32_t q) const { return (flag[q] >> 2) & 1; }
};

// the first node of every arc
__global__ __launch_bounds__(256) void simplify_arc_start_kernel(const uint8_t* __restrict__ flag, const int32_t* __restrict__ arc,
                                                                 int32_t N, int32_t* __restrict__ astart, int* __restrict__ err)
{
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (q >= N || !(flag[q] & N_ARC_START))
    return;
  const int32_t a = arc[q] - 1;
  if ((uint32_t)a >= (uint32_t)N)
    atomicOr(err, 32);
  else
    astart[a] = (int32_t)q;
}

// The segment of every node is its arc: from the arc's start to the next arc start, which for the last arc of a ring is
// the ring's first node.  Arc starts are kept.  The largest node count of an arc, both ends included.
__global__ __launch_bounds__(256) void simplify_seg_init_kernel(const uint8_t* __restrict__ flag, const int32_t* __restrict__ arc,
                                                                const int32_t* __restrict__ astart, const int32_t* __restrict__ ring,
                                                                const int32_t* __restrict__ noff, int32_t N, int32_t nr,
                                                                int2* __restrict__ seg, unsigned long long* __restrict__ best,
                                                                unsigned long long* __restrict__ tie, uint8_t* __restrict__ forced,
                                                                int* __restrict__ max_arc, int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int64_t N64 = ((int64_t)N + 63) & ~(int64_t)63;
  const int32_t na = arc[N - 1];
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N64; q += (int64_t)gridDim.x * blockDim.x) {
    int len = 0;
    if (q < N) {
      const int32_t a = arc[q] - 1, r = ring[q];
      int2 s = make_int2(DROPPED, 0);
      if ((uint32_t)a >= (uint32_t)na || na > N || (uint32_t)r >= (uint32_t)nr) {
        atomicOr(err, 64);
      } else {
        const int32_t r0 = noff[r], r1 = noff[r + 1], L = astart[a], nxt = a + 1 < na ? astart[a + 1] : N;
        if (r0 < 0 || r0 > q || r1 <= q || r1 > N || L < r0 || L > q || nxt <= q || nxt > N) {
          atomicOr(err, 64);
        } else if (flag[q] & N_ARC_START) {
          s = make_int2(KEPT, 0);
          len = min(nxt, r1) - (int32_t)q + 1;
        } else {
          s = make_int2(L, nxt < r1 ? nxt : r0);
        }
      }
      seg[q] = s;
      best[q] = 0;
      tie[q] = ~0ull;
      forced[q] = s.x == KEPT;  // the first split of every arc is forced: its segment is named by the arc start
    }
    for (int o = 32; o > 0; o >>= 1)
      len = max(len, __shfl_down(len, o));
    if (lane == 0 && len > 0)
      atomicMax(max_arc, len);
  }
}

// ---- rounds ----------------------------------------------------------------------------------------------------------------
// c^2 * den > num * len2 in 128 bits
__device__ inline bool beyond(unsigned long long c2, unsigned long long len2, unsigned long long num, unsigned long long den)
{
  const unsigned long long ah = __umul64hi(c2, den), al = c2 * den, bh = __umul64hi(num, len2), bl = num * len2;
  return ah > bh || (ah == bh && al > bl);
}

// the segment (L, R) of an active node that takes part in this pass, checked; CLOSED: only the nodes of closed arcs
template <bool CLOSED>
__device__ inline bool takes_part(int2 s, const int32_t* __restrict__ cidx, int32_t N, int* __restrict__ err)
{
  if (s.x < 0)
    return false;
  if (s.x >= N || (uint32_t)s.y >= (uint32_t)N) {
    atomicOr(err, 128);
    return false;
  }
  return !CLOSED || cidx[s.x] == cidx[s.y];
}

// The measure of every node that takes part -- c^2 against its segment, in the closed pass the squared distance from the
// arc's start -- and its maximum per segment.  The nodes of a segment are neighbours in the node arrays: one atomic per run.
template <bool CLOSED>
__global__ __launch_bounds__(256) void simplify_measure_kernel(const int2* __restrict__ seg, const int2* __restrict__ xy,
                                                               const int32_t* __restrict__ cidx, int32_t N,
                                                               unsigned long long* __restrict__ c2, unsigned long long* __restrict__ best,
                                                               int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int64_t N64 = ((int64_t)N + 63) & ~(int64_t)63;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N64; q += (int64_t)gridDim.x * blockDim.x) {
    int32_t key = -1;
    unsigned long long m = 0;
    if (q < N) {
      const int2 s = seg[q];
      if (takes_part<CLOSED>(s, cidx, N, err)) {
        const int2 P = xy[q], S = xy[s.x], E = xy[s.y];
        if (CLOSED) {
          const long long dx = P.x - S.x, dy = P.y - S.y;
          m = (unsigned long long)(dx * dx + dy * dy);
        } else {
          const long long c = (long long)(E.x - S.x) * (P.y - S.y) - (long long)(E.y - S.y) * (P.x - S.x);
          m = (unsigned long long)(c * c);
        }
        key = s.x;
        c2[q] = m;
      }
    }
    const int32_t prev = __shfl_up(key, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != key);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    BS_SEG_SCAN(m, BS_OP_MAX)
    if (lane == tl && key >= 0 && m > 0)
      atomicMax(best + key, m);
  }
}

// among the nodes that reach their segment's maximum, the lowest (corner << 32) | place
template <bool CLOSED>
__global__ __launch_bounds__(256) void simplify_tie_kernel(const int2* __restrict__ seg, const int32_t* __restrict__ cidx,
                                                           const unsigned long long* __restrict__ c2,
                                                           const unsigned long long* __restrict__ best, int32_t N,
                                                           unsigned long long* __restrict__ tie, int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int64_t N64 = ((int64_t)N + 63) & ~(int64_t)63;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N64; q += (int64_t)gridDim.x * blockDim.x) {
    int32_t key = -1;
    unsigned long long t = ~0ull;
    if (q < N) {
      const int2 s = seg[q];
      if (takes_part<CLOSED>(s, cidx, N, err)) {
        key = s.x;
        if (c2[q] == best[s.x])
          t = ((unsigned long long)(uint32_t)cidx[q] << 32) | (uint32_t)q;
      }
    }
    const int32_t prev = __shfl_up(key, 1);
    const unsigned long long heads = __ballot(lane == 0 || prev != key);
    const int hl = head_lane(heads, lane), tl = tail_lane(heads, lane);
    BS_SEG_SCAN(t, BS_OP_MIN)
    if (lane == tl && key >= 0 && t != ~0ull)
      atomicMin(tie + key, t);
  }
}

// The decision of every node, into the other buffers: the picked node of a segment that splits is kept, the other nodes
// of that segment move to one of its halves, the nodes of a segment that does not split are dropped.  A segment splits in
// the closed pass always; in the first round after it where `forced` marks its left end iff its maximum is above 0;
// otherwise iff the maximum is beyond the tolerance.  The next round's maxima and ties are reset for every node.
template <bool CLOSED>
__global__ __launch_bounds__(256) void simplify_decide_kernel(const int2* __restrict__ seg, const int2* __restrict__ xy,
                                                              const int32_t* __restrict__ cidx,
                                                              const unsigned long long* __restrict__ best,
                                                              const unsigned long long* __restrict__ tie,
                                                              const uint8_t* __restrict__ forced_in, int32_t N,
                                                              unsigned long long num, unsigned long long den,
                                                              int2* __restrict__ seg2, unsigned long long* __restrict__ best2,
                                                              unsigned long long* __restrict__ tie2, uint8_t* __restrict__ forced_out,
                                                              int* __restrict__ changed, int* __restrict__ err)
{
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < N; q += (int64_t)gridDim.x * blockDim.x) {
    int2 s = seg[q];
    if (takes_part<CLOSED>(s, cidx, N, err)) {
      const unsigned long long b = best[s.x];
      bool split = true;
      if (!CLOSED) {
        if (forced_in && forced_in[s.x]) {
          split = b > 0;
        } else {
          const int2 S = xy[s.x], E = xy[s.y];
          const long long dx = E.x - S.x, dy = E.y - S.y;
          split = beyond(b, (unsigned long long)(dx * dx + dy * dy), num, den);
        }
      }
      if (!split) {
        s.x = DROPPED;
      } else {
        const unsigned long long t = tie[s.x];
        const int32_t pick = (int32_t)(t & 0xFFFFFFFFull);
        if (t == ~0ull || (uint32_t)pick >= (uint32_t)N) {
          atomicOr(err, 256);
          s.x = DROPPED;
        } else if (pick == (int32_t)q) {
          if (CLOSED) {
            forced_out[s.x] = 1;
            forced_out[q] = 1;
          }
          s.x = KEPT;
          *changed = 1;
        } else if (q < pick) {
          s.y = pick;
        } else {
          s.x = pick;
        }
      }
    }
    seg2[q] = s;
    best2[q] = 0;
    tie2[q] = ~0ull;
  }
}

// ---- rings -----------------------------------------------------------------------------------------------------------------
struct KeptFlag {  // 0 for the entry behind the last
  const int2* seg;
  int32_t N;
  __host__ __device__ int32_t operator()(int32_t q) const { return q < N && seg[q].x == KEPT; }
};

__global__ __launch_bounds__(256) void simplify_ring_offsets_kernel(const int32_t* __restrict__ kscan, RingFig F, int32_t nr,
                                                                    int32_t N, int* __restrict__ err)
{
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r > nr)
    return;
  const int32_t o = F.noff[r];
  if ((uint32_t)o > (uint32_t)N) {
    atomicOr(err, 512);
    F.soff[r] = 0;
  } else {
    F.soff[r] = kscan[o];
  }
}

struct FinalArrays {  // per kept vertex in the order of the result, device
  int2* xy;
  int32_t* z;
  int32_t* right;
  int32_t* ring;
  uint8_t* flag;
};

// A kept node's number among the kept nodes of its ring in the rotated order, minus the kept nodes in front of h0's place
// there, modulo the ring's kept count: its place in walk order from h0.
__global__ __launch_bounds__(256) void simplify_final_kernel(const int2* __restrict__ seg, const int32_t* __restrict__ kscan,
                                                             NodeArrays A, RingFig F, int32_t N, int32_t nr, bool has_z,
                                                             FinalArrays O, int* __restrict__ err)
{
  const int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (q >= N || seg[q].x != KEPT)
    return;
  const int32_t r = A.ring[q];
  if ((uint32_t)r >= (uint32_t)nr) {
    atomicOr(err, 1024);
    return;
  }
  const int32_t r0 = F.noff[r], r1 = F.noff[r + 1], rot = F.rot[r];
  if (r0 < 0 || r0 > q || r1 <= q || r1 > N || rot < 0 || rot >= r1 - r0) {
    atomicOr(err, 1024);
    return;
  }
  const int32_t s0 = kscan[r0], kc = kscan[r1] - s0, kb = kscan[r1 - rot] - s0;
  int32_t o = kscan[q] - s0 - kb;
  if (o < 0)
    o += kc;
  const int64_t d = (int64_t)s0 + o;
  if (o < 0 || o >= kc || d < 0 || d >= N) {
    atomicOr(err, 1024);
    return;
  }
  O.xy[d] = A.xy[q];
  O.right[d] = A.right[q];
  O.ring[d] = r;
  O.flag[d] = A.flag[q] & (N_JUNCTION | N_LONE_START);
  if (has_z)
    O.z[d] = A.z[q];
}

// the shoelace sum of every ring over its kept vertices, reduced over the runs of equal ring inside a wave
__global__ __launch_bounds__(256) void simplify_area_kernel(const int2* __restrict__ xy, const int32_t* __restrict__ ring,
                                                            const int32_t* __restrict__ soff, const int32_t* __restrict__ kscan,
                                                            int32_t N, int32_t nr, unsigned long long* __restrict__ area2,
                                                            int* __restrict__ err)
{
  const int lane = threadIdx.x & 63;
  const int32_t nsv = kscan[N];
  if (nsv < 0 || nsv > N) {
    atomicOr(err, 2048);
    return;
  }
  const int64_t n64 = ((int64_t)nsv + 63) & ~(int64_t)63;
  for (int64_t d = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; d < n64; d += (int64_t)gridDim.x * blockDim.x) {
    int32_t r = -1;
    long long term = 0;
    if (d < nsv) {
      r = ring[d];
      if ((uint32_t)r >= (uint32_t)nr) {
        atomicOr(err, 2048);
        r = -1;
      } else {
        const int32_t a = soff[r], b = soff[r + 1];
        if (a < 0 || a > d || b <= d || b > nsv) {
          atomicOr(err, 2048);
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

// ---- emit ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void simplify_emit_kernel(FinalArrays O, int64_t nsv, int2* __restrict__ xy, int32_t* __restrict__ z,
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

const char* const SIMPLE_INVALID = "simplified outlines: null pointer, width or height < 1, width * height >= 2^29, n_labels < 0, "
                                   "d_top not 16-byte aligned, num outside [0, 2^31) or den outside [1, 2^31)";

bool bad_tolerance(int64_t num, int64_t den) { return num < 0 || num >= (1ll << 31) || den < 1 || den >= (1ll << 31); }

int internal(bs_ctx* ctx, int err)
{
  char msg[96];
  snprintf(msg, sizeof msg, "simplified outlines: an index left its range (phase mask 0x%x)", err);
  return fail(ctx, BS_ERR_INTERNAL, msg);
}

template <bool CLOSED>
void launch_round(hipStream_t st, int32_t N, const int2* seg, const NodeArrays& A, unsigned long long* c2, unsigned long long* best,
                  unsigned long long* tie, const uint8_t* forced_in, int64_t num, int64_t den, int2* seg2, unsigned long long* best2,
                  unsigned long long* tie2, uint8_t* forced_out, int* changed, int* err)
{
  const int g = node_grid(N);
  simplify_measure_kernel<CLOSED><<<g, 256, 0, st>>>(seg, A.xy, A.cidx, N, c2, best, err);
  simplify_tie_kernel<CLOSED><<<g, 256, 0, st>>>(seg, A.cidx, c2, best, N, tie, err);
  simplify_decide_kernel<CLOSED><<<g, 256, 0, st>>>(seg, A.xy, A.cidx, best, tie, forced_in, N, (unsigned long long)num,
                                                    (unsigned long long)den, seg2, best2, tie2, forced_out, changed, err);
}

}  // namespace

void simplify_forced_round(hipStream_t st, int32_t N, const int2* seg, const int2* xy, const int32_t* cidx,
                           unsigned long long* c2, unsigned long long* best, unsigned long long* tie, const uint8_t* forced,
                           int2* seg2, unsigned long long* best2, unsigned long long* tie2, int* changed, int* err)
{
  const NodeArrays A{const_cast<int2*>(xy), const_cast<int32_t*>(cidx), nullptr, nullptr, nullptr, nullptr};
  launch_round<false>(st, N, seg, A, c2, best, tie, forced, 0, 1, seg2, best2, tie2, nullptr, changed, err);
}

}  // namespace bs

using namespace bs;

extern "C" void bs_simple_outlines_free(struct bs_simple_outlines* s)
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

extern "C" int bs_simple_outlines_count_dev(bs_ctx* ctx, const int32_t* d_label, const int32_t* d_top, int32_t width,
                                            int32_t height, int32_t n_labels, int64_t num, int64_t den,
                                            struct bs_simple_outlines* out, struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->sp_valid = false;
  if (!d_label || !out || bad_image(width, height) || n_labels < 0 || (reinterpret_cast<uintptr_t>(d_top) & 15u) ||
      bad_tolerance(num, den))
    return fail(ctx, BS_ERR_INVALID, SIMPLE_INVALID);
  Chain ch;  // (its simplified outlines are this call's own result)
  struct bs_outlines& pl = ch.plain;
  struct bs_simple_outlines& res = ch.simple;
  int rc = bs_facet_outlines_count_dev(ctx, d_label, d_top, width, height, n_labels, &pl);
  if (rc != BS_OK)
    return rc;
  ch.has_plain = ch.has_simple = true;
  const int w = width, h = height;
  const bool has_z = d_top != nullptr;
  const int32_t nr = (int32_t)pl.n_rings;
  res.width = w;
  res.height = h;
  res.n_labels = n_labels;
  res.has_z = has_z;
  res.tol_num = (int32_t)num;
  res.tol_den = (int32_t)den;
  res.n_rings = nr;
  res.ms_outlines = pl.ms_halfedges + pl.ms_leaders + pl.ms_rank + pl.ms_rings;
  const bool ok[] = {alloc(&res.ring_label, nr),      alloc(&res.ring_area2, nr),  alloc(&res.label_ring_offset, (size_t)n_labels + 1),
                     alloc(&res.s_ring_vertices, nr), alloc(&res.s_ring_area2, nr), alloc(&res.s_ring_arcs, nr),
                     alloc(&res.s_ring_offset, (size_t)nr + 1)};
  if (!std::all_of(std::begin(ok), std::end(ok), [](bool b) { return b; }))
    return fail(ctx, BS_ERR_NOMEM, "simplified outlines: host allocation");
  memcpy(res.label_ring_offset, pl.label_ring_offset, 8 * ((size_t)n_labels + 1));
  if (nr > 0) {
    memcpy(res.ring_label, pl.ring_label, 4 * (size_t)nr);
    memcpy(res.ring_area2, pl.ring_area2, 8 * (size_t)nr);
  }
  auto hand_over = [&]() {
    ch.hand_over(nullptr, nullptr, out, plain);
    return BS_OK;
  };
  if (pl.n_half == 0) {  // no labelled pixel: no ring, every offset 0
    ctx->sp_state.N = ctx->sp_state.nr = 0;
    ctx->sp_nsv = 0;
    ctx->sp_has_z = has_z;
    ctx->sp_valid = true;
    return hand_over();
  }
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int32_t n = (int32_t)pl.n_half;
  const int R = rounds_of(pl.n_half);
  const int nb = nblk(n, 256);
  DevBuf* B = ctx->sp;
  DevBuf* OB = ctx->ol;
  Events<10> ev;
  for (auto& e : ev.e)
    BS_HIP(ctx, hipEventCreate(&e));
  hipcub::CountingInputIterator<int32_t> idx(0);
  const int32_t* hnum = OB[OL_HNUM].as<int32_t>();
  const int32_t* succ = OB[OL_SUCC].as<int32_t>();
  const uint8_t* vert = OB[OL_VERT].as<uint8_t>();
  const int32_t* slot = OB[OL_SLOT].as<int32_t>();
  const int32_t* leader = ctx->ol_leader;
  const int32_t* of_slot = ring_out_at(OB[OL_RING].p, (size_t)nr).of_slot;
  if (ctx->ol_nr != nr || !leader)
    return internal(ctx, 0x10000);

  // ---- nodes ----
  BS_HIP(ctx, B[SP_MISC].reserve(256));
  int* d_words = B[SP_MISC].as<int>();
  int* d_err = d_words + W_ERR;
  for (int b : {SP_HRIGHT, SP_HCIDX, SP_HZ, SP_NX0, SP_NX1, SP_VAL0, SP_VAL1})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)n));
  BS_HIP(ctx, B[SP_HFLAG].reserve(2 * (size_t)n));  // (the flags, and the node flag alone for the cut)
  BS_HIP(ctx, B[SP_RING].reserve(RING_FIG_BYTES * (size_t)nr + 8));
  uint8_t* hflag = B[SP_HFLAG].as<uint8_t>();
  uint8_t* isnode = hflag + n;
  int32_t* hright = B[SP_HRIGHT].as<int32_t>();
  int32_t* hcidx = B[SP_HCIDX].as<int32_t>();
  int32_t* hz = B[SP_HZ].as<int32_t>();
  int32_t* nx[2] = {B[SP_NX0].as<int32_t>(), B[SP_NX1].as<int32_t>()};
  int32_t* val[2] = {B[SP_VAL0].as<int32_t>(), B[SP_VAL1].as<int32_t>()};
  const RingFig F = ring_fig_at(B[SP_RING].p, (size_t)nr);
  hipcub::TransformInputIterator<int32_t, NodeCount, hipcub::CountingInputIterator<int32_t>> counts(idx, NodeCount{F.nodes, nr});
  auto scan_nodes = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, counts, F.noff, nr + 1, st); };
  BS_HIP(ctx, cub_room(B[SP_TMP], scan_nodes));
  BS_HIP(ctx, hipMemsetAsync(d_words, 0, 4 * W_COUNT, st));
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  simplify_nodes_kernel<<<nb, 256, 0, st>>>(d_label, d_top, hnum, vert, w, h, n, hflag, isnode, hright, hcidx, hz, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  // ---- placing: the cut, R Wyllie rounds that carry node counts, the node count and the first node of every ring ----
  int cw = 0;
  outline_cut_kernel<<<nb, 256, 0, st>>>(succ, leader, isnode, n, nx[0], val[0]);
  for (int r = 0; r < R; r++, cw ^= 1)
    outline_jump_kernel<<<nb, 256, 0, st>>>(nx[cw], val[cw], n, nx[cw ^ 1], val[cw ^ 1], d_err);
  const int32_t* suffix = val[cw];
  simplify_ring_init_kernel<<<nblk(nr, 256), 256, 0, st>>>(F, nr);
  simplify_ring_nodes_kernel<<<nb, 256, 0, st>>>(leader, slot, of_slot, suffix, nx[cw], n, nr, F.nodes, d_err);
  BS_HIP(ctx, cub_run(B[SP_TMP], scan_nodes));
  BS_HIP(ctx, hipEventRecord(ev.e[2], st));
  int h_err = 0;
  int32_t n_nodes = 0;
  BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&n_nodes, F.noff + nr, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // round trip 1: n_nodes
  BS_HIP(ctx, hipGetLastError());
  if (h_err)
    return internal(ctx, h_err);
  if (n_nodes < 4 * (int64_t)nr || n_nodes > n)
    return internal(ctx, 0x20000);
  const int32_t N = n_nodes;

  // ---- arcs ----
  BS_HIP(ctx, B[SP_NXY].reserve(8 * (size_t)N));
  for (int b : {SP_NCIDX, SP_NZ, SP_NRIGHT, SP_NRING, SP_ARC, SP_ASTART, SP_FZ, SP_FRIGHT, SP_FRING})
    BS_HIP(ctx, B[b].reserve(4 * (size_t)N));
  for (int b : {SP_NFLAG, SP_FORCED, SP_FFLAG})
    BS_HIP(ctx, B[b].reserve((size_t)N));
  for (int b : {SP_SEG0, SP_SEG1, SP_C2, SP_BEST0, SP_BEST1, SP_TIE0, SP_TIE1, SP_FXY})
    BS_HIP(ctx, B[b].reserve(8 * (size_t)N));
  BS_HIP(ctx, B[SP_KSCAN].reserve(4 * ((size_t)N + 1)));
  const NodeArrays A{B[SP_NXY].as<int2>(), B[SP_NCIDX].as<int32_t>(), B[SP_NZ].as<int32_t>(), B[SP_NRIGHT].as<int32_t>(),
                     B[SP_NRING].as<int32_t>(), B[SP_NFLAG].as<uint8_t>()};
  const FinalArrays O{B[SP_FXY].as<int2>(), B[SP_FZ].as<int32_t>(), B[SP_FRIGHT].as<int32_t>(), B[SP_FRING].as<int32_t>(),
                      B[SP_FFLAG].as<uint8_t>()};
  int32_t* arc = B[SP_ARC].as<int32_t>();
  int32_t* astart = B[SP_ASTART].as<int32_t>();
  int2* seg[2] = {B[SP_SEG0].as<int2>(), B[SP_SEG1].as<int2>()};
  unsigned long long* c2 = B[SP_C2].as<unsigned long long>();
  unsigned long long* best[2] = {B[SP_BEST0].as<unsigned long long>(), B[SP_BEST1].as<unsigned long long>()};
  unsigned long long* tie[2] = {B[SP_TIE0].as<unsigned long long>(), B[SP_TIE1].as<unsigned long long>()};
  uint8_t* forced = B[SP_FORCED].as<uint8_t>();
  int32_t* kscan = B[SP_KSCAN].as<int32_t>();
  hipcub::TransformInputIterator<int32_t, ArcStart, hipcub::CountingInputIterator<int32_t>> starts(idx, ArcStart{A.flag});
  auto scan_arcs = [&](void* tmp, size_t& bytes) { return hipcub::DeviceScan::InclusiveSum(tmp, bytes, starts, arc, N, st); };
  auto scan_kept = [&](const int2* segs) {  // (the buffer that holds the kept flags is known after the rounds)
    hipcub::TransformInputIterator<int32_t, KeptFlag, hipcub::CountingInputIterator<int32_t>> kf(idx, KeptFlag{segs, N});
    return [=](void* tmp, size_t& bytes) { return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, kf, kscan, N + 1, st); };
  };
  BS_HIP(ctx, cub_room(B[SP_TMP], scan_arcs, scan_kept(seg[0])));
  const int NB = nblk(N, 256), g = node_grid(N);
  simplify_ring_figures_kernel<<<node_grid(n), 256, 0, st>>>(hflag, hcidx, leader, slot, of_slot, suffix, F.nodes, n, nr, F.junctions,
                                                           F.first_junction, F.lowest, d_err);
  simplify_rot_kernel<<<nblk(nr, 256), 256, 0, st>>>(F, nr, d_err);
  simplify_scatter_kernel<<<nb, 256, 0, st>>>(hflag, hcidx, hright, hz, leader, slot, of_slot, suffix, F, w, n, nr, N, has_z, A, d_err);
  BS_HIP(ctx, cub_run(B[SP_TMP], scan_arcs));
  simplify_arc_start_kernel<<<NB, 256, 0, st>>>(A.flag, arc, N, astart, d_err);
  simplify_seg_init_kernel<<<g, 256, 0, st>>>(A.flag, arc, astart, A.ring, F.noff, N, nr, seg[0], best[0], tie[0], forced,
                                              d_words + W_MAXARC, d_err);
  int cur = 0;
  launch_round<true>(st, N, seg[0], A, c2, best[0], tie[0], nullptr, num, den, seg[1], best[1], tie[1], forced, d_words + W_CHANGED,
                     d_err);
  cur = 1;
  BS_HIP(ctx, hipEventRecord(ev.e[3], st));
  // ---- rounds: until one keeps nothing; the words are read every ROUND_BATCH rounds ----
  int64_t rounds = 0;
  bool first = true, done = false;
  while (!done) {
    if (rounds > N)
      return internal(ctx, 0x40000);  // (every counted round keeps a node: more rounds than nodes cannot be)
    BS_HIP(ctx, hipMemsetAsync(d_words + W_CHANGED, 0, 4 * ROUND_BATCH, st));
    for (int j = 0; j < ROUND_BATCH; j++, cur ^= 1, first = false)
      launch_round<false>(st, N, seg[cur], A, c2, best[cur], tie[cur], first ? forced : nullptr, num, den, seg[cur ^ 1], best[cur ^ 1],
                          tie[cur ^ 1], nullptr, d_words + W_CHANGED + j, d_err);
    int h_changed[ROUND_BATCH];
    BS_HIP(ctx, hipMemcpyAsync(h_changed, d_words + W_CHANGED, 4 * ROUND_BATCH, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, st));
    BS_HIP(ctx, hipStreamSynchronize(st));
    BS_HIP(ctx, hipGetLastError());
    if (h_err)
      return internal(ctx, h_err);
    for (int j = 0; j < ROUND_BATCH && !done; j++) {
      if (h_changed[j])
        rounds++;
      else
        done = true;
    }
  }
  BS_HIP(ctx, hipEventRecord(ev.e[4], st));
  // ---- rings: the kept flags scanned, the place of every kept vertex, area2 ----
  BS_HIP(ctx, cub_run(B[SP_TMP], scan_kept(seg[cur])));
  simplify_ring_offsets_kernel<<<nblk((int64_t)nr + 1, 256), 256, 0, st>>>(kscan, F, nr, N, d_err);
  simplify_final_kernel<<<NB, 256, 0, st>>>(seg[cur], kscan, A, F, N, nr, has_z, O, d_err);
  simplify_area_kernel<<<g, 256, 0, st>>>(O.xy, O.ring, F.soff, kscan, N, nr, F.area2, d_err);
  BS_HIP(ctx, hipEventRecord(ev.e[5], st));
  std::vector<int32_t> i32(2 * (size_t)nr + 1);
  int32_t* h_soff = i32.data();  // [nr + 1]
  int32_t* h_junc = h_soff + nr + 1;
  int h_words[W_COUNT] = {};
  int32_t n_arcs = 0;
  BS_HIP(ctx, hipMemcpyAsync(h_words, d_words, 4 * W_COUNT, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(&n_arcs, arc + N - 1, 4, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_soff, F.soff, 4 * ((size_t)nr + 1), hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(h_junc, F.junctions, 4 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipMemcpyAsync(res.s_ring_area2, F.area2, 8 * (size_t)nr, hipMemcpyDeviceToHost, st));
  BS_HIP(ctx, hipStreamSynchronize(st));  // the last round trip: n_svertices and the ring arrays
  BS_HIP(ctx, hipGetLastError());
  if (h_words[W_ERR])
    return internal(ctx, h_words[W_ERR]);
  int64_t junctions = 0, arcs = 0;
  for (int32_t r = 0; r < nr; r++) {
    res.s_ring_offset[r] = h_soff[r];
    res.s_ring_vertices[r] = h_soff[r + 1] - h_soff[r];
    res.s_ring_arcs[r] = std::max(h_junc[r], 1);
    junctions += h_junc[r];
    arcs += res.s_ring_arcs[r];
    if (res.s_ring_vertices[r] < 2)  // (two junction nodes are the least a ring can keep)
      return internal(ctx, 0x80000);
  }
  res.s_ring_offset[nr] = h_soff[nr];
  if (h_soff[0] != 0 || h_soff[nr] > N || arcs != n_arcs)
    return internal(ctx, 0x100000);
  res.n_nodes = N;
  res.n_junction_nodes = junctions;
  res.n_arcs = n_arcs;
  res.n_svertices = h_soff[nr];
  res.rounds = rounds;
  res.max_arc_nodes = h_words[W_MAXARC];
  res.ms_nodes = ev.ms(0, 1);
  res.ms_placing = ev.ms(1, 2);
  res.ms_arcs = ev.ms(2, 3);
  res.ms_rounds = ev.ms(3, 4);
  res.ms_rings = ev.ms(4, 5);
  bs_ctx::SimplifyState& S = ctx->sp_state;  // for bs_uncross.hip
  S.N = N;
  S.nr = nr;
  S.cur = cur;
  for (int j = 0; j < 2; j++)
    S.seg[j] = seg[j], S.best[j] = best[j], S.tie[j] = tie[j];
  S.c2 = c2;
  S.forced = forced;
  S.xy = A.xy, S.cidx = A.cidx, S.z = A.z, S.right = A.right, S.ring = A.ring, S.flag = A.flag;
  S.noff = F.noff, S.rot = F.rot;
  ctx->sp_nsv = res.n_svertices;
  ctx->sp_has_z = has_z;
  ctx->sp_valid = true;
  return hand_over();
}

extern "C" int bs_simple_outlines_emit_dev(bs_ctx* ctx, int32_t* d_sxy, int32_t* d_sz, int32_t* d_right, uint8_t* d_flag)
{
  if (!ctx)
    return BS_ERR_INVALID;
  if (!ctx->sp_valid)
    return fail(ctx, BS_ERR_INVALID, "simplified outlines: emit without a successful count on this context");
  const int64_t nsv = ctx->sp_nsv;
  if ((nsv > 0 && (!d_sxy || !d_right || !d_flag)) || (nsv > 0 && ctx->sp_has_z && !d_sz) || (!ctx->sp_has_z && d_sz))
    return fail(ctx, BS_ERR_INVALID,
                "simplified outlines: emit needs d_sxy, d_right and d_flag, and d_sz exactly when the count had a top image");
  ctx->sp_ms_emit = 0;
  if (nsv == 0)
    return BS_OK;
  BS_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf* B = ctx->sp;
  Events<2> ev;
  BS_HIP(ctx, hipEventCreate(&ev.e[0]));
  BS_HIP(ctx, hipEventCreate(&ev.e[1]));
  const FinalArrays O{B[SP_FXY].as<int2>(), B[SP_FZ].as<int32_t>(), B[SP_FRIGHT].as<int32_t>(), B[SP_FRING].as<int32_t>(),
                      B[SP_FFLAG].as<uint8_t>()};
  BS_HIP(ctx, hipEventRecord(ev.e[0], st));
  simplify_emit_kernel<<<node_grid(nsv), 256, 0, st>>>(O, nsv, reinterpret_cast<int2*>(d_sxy), d_sz, d_right, d_flag);
  BS_HIP(ctx, hipEventRecord(ev.e[1], st));
  BS_HIP(ctx, hipStreamSynchronize(st));
  BS_HIP(ctx, hipGetLastError());
  ctx->sp_ms_emit = ev.ms(0, 1);
  return BS_OK;
}

extern "C" int bs_simple_outlines(bs_ctx* ctx, const int32_t* label, const int32_t* top, int32_t width, int32_t height,
                                  int32_t n_labels, int64_t num, int64_t den, struct bs_simple_outlines* out,
                                  struct bs_outlines* plain)
{
  if (!ctx)
    return BS_ERR_INVALID;
  ctx->sp_valid = false;
  if (!label || !out || bad_image(width, height) || n_labels < 0 || bad_tolerance(num, den))
    return fail(ctx, BS_ERR_INVALID, SIMPLE_INVALID);
  const size_t npix = (size_t)width * height;
  DevBuf* B = ctx->sp;
  Staging S(ctx);
  const int32_t* d_label = S.upload(B[SP_IN_LABEL], label, npix);
  const int32_t* d_top = S.upload(B[SP_IN_TOP], top, 4 * npix);
  if (!S.ok())
    return S.status();
  Chain ch;  // (its simplified outlines are this call's own result)
  int rc = bs_simple_outlines_count_dev(ctx, d_label, d_top, width, height, n_labels, num, den, &ch.simple, &ch.plain);
  if (rc != BS_OK)
    return rc;
  ch.has_plain = ch.has_simple = true;
  rc = kept_vertices_to_host(ctx, S, ch.simple, {B[SP_OUT_XY], B[SP_OUT_Z], B[SP_OUT_RIGHT], B[SP_OUT_FLAG]},
                             bs_simple_outlines_emit_dev, &ctx->sp_ms_emit, "simplified outlines: host allocation");
  if (rc != BS_OK)
    return rc;
  ch.hand_over(nullptr, nullptr, out, plain);
  return BS_OK;
}

// The format is written down in include/bs_api.h.
extern "C" int bs_simple_outlines_write_obj(const struct bs_simple_outlines* o, int32_t bin, const int32_t* origin, const char* path)
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
  fprintf(fo, "# simplified outlines: %d labels, %lld rings, %lld vertices, tol2 %d/%d\n", o->n_labels, (long long)o->n_rings,
          (long long)o->n_svertices, o->tol_num, o->tol_den);
  return write_kept_rings(fo, o, bin, origin);
}
