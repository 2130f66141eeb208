// bs_host.h -- the small host helpers that every stage file used to define for itself: launch sizes, the events of a call's
// timings, the zeroed host arrays of a result, the temporary storage of a hipCUB call (cub_room, cub_run), the staging of a
// host entry point through the context's buffers (Staging) and the device mesh of the two solid stages (DevMesh).  Everything
// is internal to a translation unit.
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

// The temporary storage of a hipCUB call.  An operation is written once, as a callable hipError_t op(void* tmp, size_t& bytes)
// that hands its two parameters to the hipcub::Device... call as the first two arguments.  cub_room sizes a slot ahead for
// every operation it will hold (where the stage makes room for its other buffers); cub_run asks the operation again, with the
// arguments it is about to run with, grows a slot that is short (DevBuf::reserve returns at once where it is not) and runs.
template <class... Ops>
hipError_t cub_room(DevBuf& tmp, Ops&&... ops)
{
  size_t need = 256;
  hipError_t e = hipSuccess;
  auto ask = [&](auto&& op) {
    size_t bytes = 0;
    hipError_t r = op(nullptr, bytes);
    need = std::max(need, bytes);
    if (e == hipSuccess)
      e = r;
  };
  (ask(ops), ...);
  return e != hipSuccess ? e : tmp.reserve(need);
}

template <class Op>
hipError_t cub_run_sized(DevBuf& tmp, Op&& op)  // the slot as cub_room sized it for this very callable: no second question
{
  size_t bytes = tmp.cap;
  return op(tmp.p, bytes);
}

template <class Op>
hipError_t cub_run(DevBuf& tmp, Op&& op)
{
  hipError_t e = cub_room(tmp, op);
  return e != hipSuccess ? e : cub_run_sized(tmp, op);
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

// The staging of a host entry point through the context's DevBuf slots: select the device, upload the inputs, make room for
// the outputs, call the _dev form, download what the caller asked for, finish.  The first HIP error sticks and every later
// step does nothing, so a host form checks ok() once before the device call and returns finish() at its end; either reports
// BS_ERR_HIP through fail() with the step's name and the HIP error string.
struct Staging {
  bs_ctx* ctx;
  hipError_t e;
  const char* what = "host staging: hipSetDevice";

  explicit Staging(bs_ctx* c) : ctx(c), e(hipSetDevice(c->device)) {}
  bool ok() const { return e == hipSuccess; }
  int status() const { return ok() ? BS_OK : fail(ctx, BS_ERR_HIP, what, e); }
  hipError_t step(hipError_t r, const char* name)
  {
    if (r != hipSuccess)
      what = name;
    return r;
  }

  // n elements of T in slot b; nullptr, and nothing reserved, where the output is not wanted
  template <class T>
  T* room(DevBuf& b, size_t n, bool wanted = true)
  {
    if (!wanted || !ok() || (e = step(b.reserve(sizeof(T) * n), "host staging: room")) != hipSuccess)
      return nullptr;
    return b.as<T>();
  }
  // room for n elements and their copy from the host; an optional input that is NULL stays NULL on the device
  template <class T>
  T* upload(DevBuf& b, const T* host, size_t n)
  {
    T* d = room<T>(b, n, host != nullptr);
    if (d)
      e = step(hipMemcpyAsync(d, host, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream), "host staging: upload");
    return d;
  }
  // n elements back to the host where the caller gave a place for them
  template <class T>
  void download(T* host, const T* dev, size_t n)
  {
    if (host && n && ok())
      e = step(hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, ctx->stream), "host staging: download");
  }
  int finish()
  {
    if (ok())
      e = step(hipStreamSynchronize(ctx->stream), "host staging: finish");
    return status();
  }
};

// The device mesh of the two solid stages in one slot: vertex (4 int32 each) | face_offset [nf + 1] | face_index [ni] |
// face_building [nf] | face_kind [nf], each 16-byte aligned, and 16 bytes of slack.
struct DevMesh {
  size_t nv, nf, ni;
  int32_t *vertex = nullptr, *face_offset = nullptr, *face_index = nullptr, *face_building = nullptr;
  uint8_t* face_kind = nullptr;

  DevMesh(int64_t n_vertices, int64_t n_faces, int64_t n_indices) : nv((size_t)n_vertices), nf((size_t)n_faces), ni((size_t)n_indices) {}
  static size_t up(size_t b) { return (b + 15) & ~(size_t)15; }
  size_t bytes() const { return up(16 * nv) + up(4 * (nf + 1)) + up(4 * ni) + up(4 * nf) + up(nf) + 16; }
  void place(char* d)  // (nullptr where the room failed: the caller checks the staging before it uses the mesh)
  {
    if (!d)
      return;
    vertex = reinterpret_cast<int32_t*>(d);
    face_offset = reinterpret_cast<int32_t*>(d += up(16 * nv));
    face_index = reinterpret_cast<int32_t*>(d += up(4 * (nf + 1)));
    face_building = reinterpret_cast<int32_t*>(d += up(4 * ni));
    face_kind = reinterpret_cast<uint8_t*>(d += up(4 * nf));
  }
  // the five host arrays of a result (none NULL, an empty mesh's neither) and their download; false: out of host memory
  template <class R>
  bool to_host(Staging& S, R& r) const
  {
    if (!alloc(&r.vertex, 4 * nv) || !alloc(&r.face_offset, nf + 1) || !alloc(&r.face_index, ni) ||
        !alloc(&r.face_building, nf) || !alloc(&r.face_kind, nf))
      return false;
    S.download(r.vertex, vertex, 4 * nv);
    S.download(r.face_offset, face_offset, nf + 1);
    S.download(r.face_index, face_index, ni);
    S.download(r.face_building, face_building, nf);
    S.download(r.face_kind, face_kind, nf);
    return true;
  }
};

}  // namespace
}  // namespace bs
