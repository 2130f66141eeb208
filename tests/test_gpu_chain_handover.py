"""The hand-over contract of the chain entry points (include/bs_api.h): bs_simplified_outlines .. bs_point_residuals run the
stages before them and hand each intermediate result to an optional out-pointer.  A NULL out-pointer changes nothing else; an
error after the chain has succeeded leaves every out struct untouched and the context usable.  The entry points are driven
through _lib with ctypes; everything is an exact integer, every comparison is ==.  (No stage before the polygon solids has an
error that arises after the stages in front of it have succeeded, so (b) has no case for them.)"""
import ctypes as C
import itertools

import numpy as np
import pytest

from buildingsegment_amd import _lib

from test_modelraster_cpu import ref as mr_ref  # noqa: E402
from test_pointresid_cpu import BY_NAME, cloud, mref, pref as presid_ref, ref as pr_ref, upstream  # noqa: E402
from test_polysolid_cpu import load_polysolid_cases  # noqa: E402

poly_ref = load_polysolid_cases().pref
pytestmark = pytest.mark.gpu
RUNS = (("nested", (2, 1)), ("bay", (100, 1)))  # of tests/modelraster_ref/cases.py, with the clouds of tests/pointresid_ref
NB, BASE = 3, -1000
OK, ERR_RANGE = 0, -2
CHAIN = ("tri", "clean", "simple", "plain")  # the order of the out-pointers
TYPES = {"tri": _lib.OutlineTriangles, "clean": _lib.CleanOutlines, "simple": _lib.SimpleOutlines, "plain": _lib.Outlines}
OUTLINE = lambda s: dict(ring_label=s.n_rings, ring_area2=s.n_rings, s_ring_vertices=s.n_rings, s_ring_area2=s.n_rings,  # noqa: E731
                         s_ring_arcs=s.n_rings, s_ring_offset=s.n_rings + 1, label_ring_offset=s.n_labels + 1, sxy=2 * s.n_svertices,
                         sz=s.n_svertices, s_right=s.n_svertices, s_flag=s.n_svertices)
LENGTHS = {  # the entries of every array of a struct
    _lib.Outlines: lambda s: dict(ring_label=s.n_rings, ring_start=s.n_rings, ring_length=s.n_rings, ring_vertices=s.n_rings,
                                  ring_area2=s.n_rings, ring_bbox=4 * s.n_rings, ring_offset=s.n_rings + 1,
                                  label_ring_offset=s.n_labels + 1, xy=2 * s.n_vertices, z=s.n_vertices),
    _lib.SimpleOutlines: OUTLINE,
    _lib.CleanOutlines: OUTLINE,
    _lib.OutlineTriangles: lambda s: dict(tri_offset=s.n_labels + 1, label_status=s.n_labels, label_area2=s.n_labels,
                                          label_tests=s.n_labels, bridge=2 * s.n_rings, tri=3 * s.n_triangles),
    _lib.PolySolids: lambda s: dict({k: s.n_buildings for k, _ in _lib.POLY_FIGURES}, vertex=4 * s.n_vertices,
                                    face_offset=s.n_faces + 1, face_index=s.n_indices, face_building=s.n_faces, face_kind=s.n_faces),
    _lib.ModelRaster: lambda s: {k: s.n_labels for k in _lib.MRASTER_FIGURES},
    _lib.PointResiduals: lambda s: {k: s.n_labels for k in _lib.PRESID_FIGURES},
}
FREE = {_lib.Outlines: "bs_outlines_free", _lib.SimpleOutlines: "bs_simple_outlines_free", _lib.CleanOutlines: "bs_clean_outlines_free",
        _lib.OutlineTriangles: "bs_outline_triangles_free", _lib.PolySolids: "bs_poly_solids_free",
        _lib.ModelRaster: "bs_model_raster_free", _lib.PointResiduals: "bs_point_residuals_free"}


def contents(s):
    """every scalar of a struct but its timings, and the bytes of every array (None for a NULL pointer)"""
    lengths = LENGTHS[type(s)](s)
    out = {}
    for name, ct in s._fields_:
        v = getattr(s, name)
        if ct is C.c_double:
            assert name.startswith("ms_")
        elif name in lengths:
            out[name] = C.string_at(v, lengths[name] * C.sizeof(ct._type_)) if v else None
        else:
            out[name] = int(v)
    assert set(lengths) <= set(out)
    return out


def take(L, s):
    """the contents of a struct the library filled, which is then freed: the free leaves it zeroed"""
    got = contents(s)
    getattr(L, FREE[type(s)])(C.byref(s))
    assert bytes(s) == bytes(C.sizeof(s))
    return got


def ptr(a):
    return None if a is None else a.ctypes.data


def entry_points(L, h, name, tol, xyz=None, top=None, lb=None):
    """name -> (the call over the run's images with the chain out-pointers given by keyword, its result type, its optional
    out-pointers, its output arrays); xyz, top and lb replace the run's cloud, top image and building table"""
    c, _, b = BY_NAME[name]
    k = cloud(name, tol)
    label = np.ascontiguousarray(c["label"], np.int32)
    top = np.ascontiguousarray(c["top"] if top is None else top, np.int32)
    xyz = np.ascontiguousarray(k.xyz if xyz is None else xyz, np.int32)
    lb = np.ascontiguousarray(np.arange(c["n_labels"]) % NB if lb is None else lb, np.int32)
    (hh, w), nl, n = label.shape, c["n_labels"], len(xyz)
    images = [np.full((hh, w), -7, np.int32) for _ in range(3)]
    points = [np.full(n, -7, np.int32) for _ in range(3)]
    head = (h, label.ctypes.data, top.ctypes.data, w, hh, nl, tol[0], tol[1])
    keep = (label, top, xyz, lb, k)  # (the arrays live as long as the calls)

    def chain(p, *names):
        return [p.get(x) for x in names]

    return {
        "simple": (lambda out, **p: L.bs_simple_outlines(*head, out, *chain(p, "plain")), _lib.SimpleOutlines, ("plain",), [], keep),
        "clean": (lambda out, **p: L.bs_clean_outlines(*head, -1, 0, out, *chain(p, "simple", "plain")), _lib.CleanOutlines,
                  ("simple", "plain"), [], keep),
        "tri": (lambda out, **p: L.bs_outline_triangles(*head, 0, out, *chain(p, "clean", "simple", "plain")), _lib.OutlineTriangles,
                ("clean", "simple", "plain"), [], keep),
        "poly": (lambda out, **p: L.bs_poly_solids(*head, 0, lb.ctypes.data, NB, b, BASE, out, *chain(p, *CHAIN)), _lib.PolySolids,
                 CHAIN, [], keep),
        "raster": (lambda out, **p: L.bs_model_raster(*head, 0, *[ptr(i) for i in images], out, *chain(p, *CHAIN)), _lib.ModelRaster,
                   CHAIN, images, keep),
        "resid": (lambda out, **p: L.bs_point_residuals(*head, 0, xyz.ctypes.data, n, k.bin, k.plane_idx.ctypes.data,
                                                        k.label_plane.ctypes.data, k.clip2, *[ptr(a) for a in points], out,
                                                        *chain(p, *CHAIN)), _lib.PointResiduals, CHAIN, points, keep),
    }


@pytest.mark.parametrize("name,tol", RUNS)
def test_every_subset_of_null_out_pointers(gpu_ctx, name, tol):
    """(a) every subset of the optional chain out-pointers NULL: BS_OK, the stage's own result and every struct handed over
    equal those of the call with all pointers, and every struct frees cleanly"""
    L, h = gpu_ctx._L, gpu_ctx._h
    for stage, (call, result, optional, arrays, _) in entry_points(L, h, name, tol).items():
        want = None
        for r in range(len(optional), -1, -1):  # all pointers first
            for given in itertools.combinations(optional, r):
                out = result()
                structs = {x: TYPES[x]() for x in given}
                for a in arrays:
                    a.fill(-7)
                rc = call(C.byref(out), **{x: C.byref(s) for x, s in structs.items()})
                assert rc == OK, (stage, given, L.bs_last_error(h))
                got = dict({x: take(L, s) for x, s in structs.items()}, own=take(L, out), arrays=[a.copy() for a in arrays])
                if want is None:
                    want = got
                    assert tuple(given) == tuple(optional) and want["own"] and all(want[x] for x in optional)
                assert got["own"] == want["own"], (stage, given)
                assert all(np.array_equal(x, y) for x, y in zip(got["arrays"], want["arrays"])), (stage, given)
                for x in given:
                    assert got[x] == want[x], (stage, given, x)


@pytest.mark.parametrize("name,tol", RUNS)
def test_an_error_after_the_chain_leaves_every_struct(gpu_ctx, name, tol):
    """(b) the chain succeeds and the stage fails with BS_ERR_RANGE: one point at z = 2^24 (point residuals), tops of 2^24 (model
    raster: a vertex of a triangle out of range), a label_building value equal to n_buildings (polygon solids).  Every out
    struct keeps its bytes, and the next call on the context gives the restatement's result"""
    ctx = gpu_ctx
    L, h = ctx._L, ctx._h
    c, _, b = BY_NAME[name]
    k = cloud(name, tol)
    nl = c["n_labels"]
    far = k.xyz.copy()
    far[len(far) // 2, 2] = 1 << 24
    lb = np.arange(nl) % NB
    bad_lb = lb.copy()
    bad_lb[0] = NB
    bad = (("resid", dict(xyz=far), b"a point lies 2^24"), ("raster", dict(top=np.full_like(c["top"], 1 << 24)), b"2^24"),
           ("poly", dict(lb=bad_lb), b"label_building"))
    for stage, replaced, word in bad:
        call, result, optional, arrays, _ = entry_points(L, h, name, tol, **replaced)[stage]
        out = result()
        structs = {x: TYPES[x]() for x in optional}
        for s in [out] + list(structs.values()):
            C.memset(C.byref(s), 0x5A, C.sizeof(s))
        rc = call(C.byref(out), **{x: C.byref(s) for x, s in structs.items()})
        assert rc == ERR_RANGE and word in L.bs_last_error(h), (stage, rc, L.bs_last_error(h))
        for s in [out] + list(structs.values()):
            assert bytes(s) == b"\x5a" * C.sizeof(s), (stage, type(s).__name__)
        assert all((a == -7).all() for a in arrays), stage
        if stage == "resid":
            got = ctx.point_residuals(c["label"], c["top"], k.xyz, n_labels=nl, num=tol[0], den=tol[1], bin=k.bin,
                                      plane_idx=k.plane_idx, label_plane=k.label_plane, clip2=k.clip2)[0]
            diff = presid_ref.same(got, pr_ref(name, tol)[0])
        elif stage == "raster":
            got = ctx.model_raster(c["label"], c["top"], n_labels=nl, num=tol[0], den=tol[1])[0]
            diff = mref.same(got, mr_ref(name, tol)[0])
        else:
            got = ctx.poly_solids(c["label"], c["top"], lb.astype(np.int32), n_labels=nl, n_buildings=NB, num=tol[0], den=tol[1],
                                  bin=b, base_z=BASE)[0]
            diff = poly_ref.same(got, poly_ref.poly_solids(*upstream(name, tol), lb, NB, b, BASE))
        assert diff is None, (stage, diff)
