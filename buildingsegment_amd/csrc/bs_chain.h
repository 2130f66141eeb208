// bs_chain.h -- the intermediate results of a chain call (outlines -> simplified -> clean -> triangles) and their hand-over.
// An entry point lets the stage before it fill the structs it needs, sets their flags, and either hands everything over at
// its end or returns early: whatever was filled and not handed over is freed.  The out-pointers are written by hand_over
// alone, so that an error leaves them untouched.  Beside it the image limit that the chain's stages share, and what the
// simplified and the clean outlines share on the host: the download of their kept vertices and the body of their OBJ.
// Everything is internal to a translation unit.
#pragma once

#include <cstdio>
#include <cstring>

#include "bs_host.h"

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

// The kept vertices of the simplified and of the clean outlines, whose structs end alike (sxy, sz, s_right, s_flag): the host
// arrays, room in the stage's four output slots, the stage's emit, the download.
struct KeptSlots {
  DevBuf &xy, &z, &right, &flag;
};

template <class R>
int kept_vertices_to_host(bs_ctx* ctx, Staging& S, R& res, KeptSlots out,
                          int (*emit)(bs_ctx*, int32_t*, int32_t*, int32_t*, uint8_t*), const double* ms_emit, const char* no_memory)
{
  const bool has_z = res.has_z != 0;
  const size_t nv = (size_t)res.n_svertices;
  if (!alloc(&res.sxy, 2 * nv) || (has_z && !alloc(&res.sz, nv)) || !alloc(&res.s_right, nv) || !alloc(&res.s_flag, nv))
    return fail(ctx, BS_ERR_NOMEM, no_memory);
  if (nv == 0)
    return BS_OK;
  int32_t* d_xy = S.room<int32_t>(out.xy, 2 * nv);
  int32_t* d_z = S.room<int32_t>(out.z, nv);  // (reserved without a top image too)
  int32_t* d_right = S.room<int32_t>(out.right, nv);
  uint8_t* d_flag = S.room<uint8_t>(out.flag, nv);
  if (!S.ok())
    return S.status();
  int rc = emit(ctx, d_xy, has_z ? d_z : nullptr, d_right, d_flag);
  if (rc != BS_OK)
    return rc;
  S.download(res.sxy, d_xy, 2 * nv);
  S.download(res.sz, d_z, nv);  // (sz is NULL without a top image)
  S.download(res.s_right, d_right, nv);
  S.download(res.s_flag, d_flag, nv);
  rc = S.finish();
  if (rc == BS_OK)
    res.ms_emit = *ms_emit;
  return rc;
}

// the OBJ of either struct after the writer's own first line: a group, the vertices and one closed line per ring; closes fo
template <class R>
int write_kept_rings(FILE* fo, const R* o, int32_t bin, const int32_t* origin)
{
  const int64_t org[3] = {origin ? origin[0] : 0, origin ? origin[1] : 0, origin ? origin[2] : 0};
  for (int64_t r = 0; r < o->n_rings; r++) {
    const int32_t l = o->ring_label[r];
    fprintf(fo, "g label_%d_ring_%lld_%s\n", l, (long long)(r - o->label_ring_offset[l]), o->ring_area2[r] > 0 ? "outer" : "hole");
    const int64_t a = o->s_ring_offset[r], b = o->s_ring_offset[r + 1];
    for (int64_t v = a; v < b; v++)
      fprintf(fo, "v %lld %lld %lld\n", (long long)((int64_t)o->sxy[2 * v] * bin + org[0]),
              (long long)((int64_t)o->sxy[2 * v + 1] * bin + org[1]), (long long)((o->sz ? (int64_t)o->sz[v] : 0) + org[2]));
    fputs("l", fo);
    for (int64_t v = a; v < b; v++)
      fprintf(fo, " %lld", (long long)(v + 1));
    fprintf(fo, " %lld\n", (long long)(a + 1));
  }
  const bool ok = !ferror(fo);
  return (fclose(fo) == 0 && ok) ? BS_OK : BS_ERR_INVALID;
}

}  // namespace
}  // namespace bs
