// bs_uf.h -- lock-free union-find on a parent array with parent[x] <= x, shared by the kNN-graph components
// (bs_shard.hip) and the raster components of the footprint tracer (bs_contour.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bs {

// Union-find on a parent array over GLOBAL point ids; invariant parent[x] <= x, roots point at themselves, a
// pointer only ever moves to a smaller member of the same component (so a stale read is still an ancestor).
// Loads go to L2 (agent scope): CUs do not see each other's stores through their L1.
__device__ inline int32_t uf_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int32_t uf_find(int32_t* parent, int32_t x)
{
  int32_t p = uf_load(parent + x);
  while (p != x) {
    const int32_t gp = uf_load(parent + p);
    if (gp != p)  // path halving; racing writers only ever store smaller ancestors
      __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = p;
    p = gp;
  }
  return x;
}

// hook the larger root under the smaller one (ECL-CC style); returns true iff THIS call performed a union
__device__ inline bool uf_union(int32_t* parent, int32_t u, int32_t v)
{
  int32_t ru = uf_find(parent, u), rv = uf_find(parent, v);
  while (ru != rv) {
    const int32_t hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    const int32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi)
      return true;
    // hi stopped being a root in the meantime: continue from where it points now
    ru = uf_find(parent, old);
    rv = lo;
  }
  return false;
}

}  // namespace bs
