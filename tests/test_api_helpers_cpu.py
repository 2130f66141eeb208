"""The binding's shared helpers on ctypes pointers taken from numpy arrays: _copy, _copy_arrays, _fill, _take_mesh and
_take_chain.  No GPU, no library."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest

from buildingsegment_amd import _lib, api


def ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


@pytest.mark.parametrize("n", [0, 1, 3])
@pytest.mark.parametrize("dt,ct,cols", [(np.int32, C.c_int32, 1), (np.int32, C.c_int32, 2), (np.uint8, C.c_uint8, 1),
                                        (np.int64, C.c_int64, 1), (np.float64, C.c_double, 3)])
def test_copy(n, dt, ct, cols):
    shape = (n, cols) if cols > 1 else (n,)
    src = (np.arange(max(n * cols, 1)) + 7).astype(dt)  # (never an empty buffer under the pointer)
    want = src[:n * cols].reshape(shape).copy()
    got = api._copy(ptr(src, ct), shape, dt)
    assert got.dtype == dt and got.shape == shape and got.flags.owndata and np.array_equal(got, want)
    src[:] = 0  # the copy does not alias the source
    assert np.array_equal(got, want)


def test_copy_refuses_another_dtype():
    with pytest.raises(TypeError):
        api._copy(ptr(np.zeros(2, np.int64), C.c_int64), (2,), np.int32)


@pytest.mark.parametrize("n", [0, 1, 3])
def test_copy_arrays(n):
    src = {"ring_label": np.arange(max(n, 1), dtype=np.int32), "ring_bbox": np.arange(max(4 * n, 1), dtype=np.int32),
           "ring_area2": np.arange(max(n, 1), dtype=np.int64) - 5}
    out = _lib.Outlines()
    for k, a in src.items():
        setattr(out, k, ptr(a, C.c_int64 if a.dtype == np.int64 else C.c_int32))
    got = api._copy_arrays(out, (("ring_label", np.int32, 1), ("ring_bbox", np.int32, 4)) + api._rows(("ring_area2",), np.int64), n)
    assert [got[k].shape for k in src] == [(n,), (n, 4), (n,)] and [got[k].dtype for k in src] == [a.dtype for a in src.values()]
    assert all(np.array_equal(got[k].reshape(-1), a[:got[k].size]) for k, a in src.items())


@pytest.mark.parametrize("n", [0, 1, 3])
def test_fill(n):
    o = NS(ring_label=np.arange(n, dtype=np.int64), ring_bbox=np.arange(4 * n).reshape(n, 4), ring_area2=[9] * n)
    st = _lib.Outlines()
    table = [("ring_label", np.int32, n), ("ring_bbox", np.int32, 4 * n), ("ring_area2", np.int64, n)]
    keep = api._fill(st, o, "Outlines", table, [])
    assert [a.dtype for a in keep] == [np.int32, np.int32, np.int64] and bool(st.ring_label) and bool(st.ring_area2)
    assert np.array_equal(api._copy(st.ring_bbox, (n, 4), np.int32), o.ring_bbox)
    assert np.array_equal(api._copy(st.ring_area2, (n,), np.int64), o.ring_area2)
    with pytest.raises(ValueError, match="Outlines.ring_bbox must hold"):
        api._fill(st, o, "Outlines", [("ring_bbox", np.int32, 4 * n + 1)], [])


@pytest.mark.parametrize("cls", [_lib.Solids, _lib.PolySolids])
@pytest.mark.parametrize("nv,nf,ni", [(0, 0, 0), (1, 1, 1), (3, 2, 7)])
def test_take_mesh(cls, nv, nf, ni):
    src = dict(vertex=np.arange(max(4 * nv, 1), dtype=np.int32), face_offset=np.arange(nf + 1, dtype=np.int32),
               face_index=np.arange(max(ni, 1), dtype=np.int32), face_building=np.arange(max(nf, 1), dtype=np.int32),
               face_kind=np.arange(max(nf, 1), dtype=np.uint8))
    out = cls()
    out.n_vertices, out.n_faces, out.n_indices = nv, nf, ni
    for k, a in src.items():
        setattr(out, k, ptr(a, C.c_uint8 if a.dtype == np.uint8 else C.c_int32))
    got = api._take_mesh(out)
    want = dict(vertex=src["vertex"][:4 * nv].reshape(nv, 4), face_offset=src["face_offset"], face_index=src["face_index"][:ni],
                face_building=src["face_building"][:nf], face_kind=src["face_kind"][:nf])
    assert list(got) == list(want)
    want = {k: a.copy() for k, a in want.items()}
    for a in src.values():
        a[:] = 0
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("fail_at", [None, 0, 1, 2])
def test_take_chain_frees_every_struct_once(fail_at):
    freed = []

    class L:
        def __getattr__(self, name):
            return lambda ref: freed.append((name, C.addressof(ref._obj)))

    def taker(k):
        def take(L_, st, arg):
            try:
                if k == fail_at:
                    raise MemoryError("copy")
                return (k, arg)
            finally:
                api._free(L_, st)
        return take

    structs = [_lib.OutlineTriangles(), _lib.CleanOutlines(), _lib.Outlines()]
    parts = [(taker(k), st, k * 10) for k, st in enumerate(structs)]
    if fail_at is None:
        assert api._take_chain(L(), *parts) == ((0, 0), (1, 10), (2, 20))
    else:
        with pytest.raises(MemoryError):
            api._take_chain(L(), *parts)
    assert sorted(freed) == sorted(zip(("bs_outline_triangles_free", "bs_clean_outlines_free", "bs_outlines_free"),
                                       map(C.addressof, structs)))
