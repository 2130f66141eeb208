// bs_host.h -- the small host helpers that every stage file used to define for itself: launch sizes, the events of a call's
// timings, the zeroed host arrays of a result.  Everything is internal to a translation unit.
#pragma once

#include <algorithm>
#include <cstdlib>

#include "bs_common.h"

namespace bs {
namespace {

constexpr int SWEEP_CAP = 1024;  // workgroups of a grid-stride pass

inline int nblk(int64_t n, int b) { return (int)((n + b - 1) / b); }
inline int sweep(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(nblk(n, 256), SWEEP_CAP)); }

template <int N>
struct Events {  // created by the caller one by one; whatever was created is destroyed
  hipEvent_t e[N] = {};
  ~Events()
  {
    for (auto& x : e)
      if (x)
        (void)hipEventDestroy(x);
  }
  double ms(int i, int j)
  {
    float t = 0;
    return hipEventElapsedTime(&t, e[i], e[j]) == hipSuccess ? t : 0.0;
  }
};

template <class T>
bool alloc(T** p, size_t n)
{
  *p = (T*)calloc(std::max<size_t>(n, 1), sizeof(T));
  return *p != nullptr;
}

inline int bits_of(int64_t n)  // bits that hold 0 .. n - 1 (at least 1)
{
  int b = 1;
  while (b < 32 && (1ll << b) < n)
    b++;
  return b;
}

// frees a half-built result through its own bs_..._free unless it is kept
template <class T, void (*FREE)(T*)>
struct FreeUnlessKept {
  T* r;
  bool keep = false;
  ~FreeUnlessKept()
  {
    if (!keep)
      FREE(r);
  }
};

}  // namespace
}  // namespace bs
