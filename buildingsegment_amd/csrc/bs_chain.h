// bs_chain.h -- the intermediate results of a chain call (outlines -> simplified -> clean -> triangles) and their hand-over.
// An entry point lets the stage before it fill the structs it needs, sets their flags, and either hands everything over at
// its end or returns early: whatever was filled and not handed over is freed.  The out-pointers are written by hand_over
// alone, so that an error leaves them untouched.  Beside it the image limit that the chain's stages share.
// Everything is internal to a translation unit.
#pragma once

#include <cstring>

#include "bs_common.h"

namespace bs {
namespace {

// the image limit of the whole chain, checked by every stage that takes images (a half-edge is numbered 4 * pixel + side in
// 31 bits; the stages outside the chain have other limits under this name, so it cannot live in bs_host.h)
inline bool bad_image(int32_t w, int32_t h) { return w < 1 || h < 1 || (int64_t)w * h >= (1ll << 29); }

struct Chain {
  struct bs_outlines plain;
  struct bs_simple_outlines simple;
  struct bs_clean_outlines clean;
  struct bs_outline_triangles tri;
  bool has_plain = false, has_simple = false, has_clean = false, has_tri = false;  // filled: to be freed or handed over

  Chain()
  {
    memset(&plain, 0, sizeof plain);
    memset(&simple, 0, sizeof simple);
    memset(&clean, 0, sizeof clean);
    memset(&tri, 0, sizeof tri);
  }
  Chain(const Chain&) = delete;
  Chain& operator=(const Chain&) = delete;
  ~Chain() { hand_over(nullptr, nullptr, nullptr, nullptr); }

  // every filled result moves to its out-pointer, or is freed where that is NULL
  void hand_over(struct bs_outline_triangles* t, struct bs_clean_outlines* c, struct bs_simple_outlines* s, struct bs_outlines* p)
  {
    move(tri, has_tri, t, bs_outline_triangles_free);
    move(clean, has_clean, c, bs_clean_outlines_free);
    move(simple, has_simple, s, bs_simple_outlines_free);
    move(plain, has_plain, p, bs_outlines_free);
  }

 private:
  template <class T>
  static void move(T& x, bool& filled, T* out, void (*release)(T*))
  {
    if (!filled)
      return;
    if (out)
      *out = x;
    else
      release(&x);
    filled = false;
  }
};

}  // namespace
}  // namespace bs
