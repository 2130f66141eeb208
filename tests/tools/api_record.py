#!/usr/bin/env python3
"""Records what buildingsegment_amd/api.py promises its callers, without a GPU and without the library:
  tests/data/api_surface.json   every public name of api and every public method of Context with its kind and signature,
                                every dataclass with its ordered fields and their defaults, and the private names that
                                tests and tools use;
  tests/data/api_rejects.json   for every malformed argument of _cases(): the exception type, whether the message names the
                                method, and the argument the message must name.
The rejects run on a Context made with Context.__new__: it has no handle, and in place of the library a stand-in whose every
function raises ReachedLibrary when it is CALLED, as does _lib.load() meanwhile, so a case that is not refused before the first
library call shows as ReachedLibrary.  tests/test_api_surface_cpu.py and tests/test_api_rejects_cpu.py replay both files.
usage: python tests/tools/api_record.py --write     (only ever from a commit whose api.py is the one to be held to)"""
import argparse
import dataclasses
import inspect
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from buildingsegment_amd import api  # noqa: E402

DATA = os.path.join(ROOT, "tests", "data")
PRIVATE = ("_ground_struct", "_solid_defaults", "_solid_tables", "_take_roof_generalise", "_roof_facets_struct",
           "_outlines_struct", "_FACET_ARRAYS", "_EDGE_ARRAYS", "_lib")


def _own(v):
    """the package's own classes and functions, and plain constants: not what api imports from elsewhere"""
    if inspect.isclass(v) or inspect.isfunction(v):
        return v.__module__.startswith("buildingsegment_amd")
    return isinstance(v, (int, float, str, tuple))


def _describe(v):
    if isinstance(v, (int, float, str)):
        return {"kind": type(v).__name__, "value": v}
    if inspect.isclass(v):
        kind = "class"
    elif inspect.isfunction(v) or inspect.ismethod(v):
        kind = "function"
    elif isinstance(v, tuple):
        return {"kind": "tuple", "value": [[str(np.dtype(x).name) if isinstance(x, type) else x for x in row] for row in v]}
    else:
        return {"kind": type(v).__name__}
    try:
        sig = str(inspect.signature(v))
    except (ValueError, TypeError):
        sig = None
    return {"kind": kind, "signature": sig}


def _default(f):
    if f.default is not dataclasses.MISSING:
        return repr(f.default)
    if f.default_factory is not dataclasses.MISSING:
        return "factory " + repr(f.default_factory)
    return None


def surface():
    public = {k: v for k, v in vars(api).items() if not k.startswith("_") and _own(v)}
    methods = {k: v for k, v in vars(api.Context).items() if not k.startswith("_")}
    return {"names": {k: _describe(v) for k, v in sorted(public.items())},
            "context": {k: _describe(getattr(api.Context, k)) for k in sorted(methods)},
            "dataclasses": {k: [[f.name, _default(f)] for f in dataclasses.fields(v)]
                            for k, v in sorted(public.items()) if dataclasses.is_dataclass(v)},
            "private": {k: _describe(getattr(api, k)) for k in PRIVATE}}


class ReachedLibrary(Exception):
    """a case was not refused before the first call into the library"""


class _NoLibrary:
    def __getattr__(self, name):
        def fn(*a, **k):
            raise ReachedLibrary(name)
        return fn


def bare_context():
    ctx = api.Context.__new__(api.Context)
    ctx._L, ctx._h = _NoLibrary(), None
    return ctx


I32, I64 = np.int32, np.int64
LABEL, TOP, BMAP = np.zeros((3, 4), I32), np.zeros((3, 4, 4), I32), np.zeros((3, 4), I32)
XYZ, PIDX = np.zeros((5, 3), I32), np.zeros(5, I32)
FLAT_LABEL, BAD_TOP, XY2, SHORT = np.zeros(4, I32), np.zeros((3, 4, 3), I32), np.zeros((5, 2), I32), np.zeros(4, I32)
BAD_ORIGIN = [1, 2]


def _facets(**kw):
    rf = NS(n_facets=0, n_edges=0, n_pixels=0, n_border=0, facet=LABEL,
            **{name: np.zeros((0, cols) if cols > 1 else 0, dt) for name, dt, cols in api._FACET_ARRAYS + api._EDGE_ARRAYS})
    rf.__dict__.update(kw)
    return rf


def _solids(**kw):
    return NS(**dict(dict(top=TOP, bin=100, base=None, base_z=0, n_buildings=0, vertex=np.zeros((0, 4), I32),
                          face_offset=np.zeros(1, I32), face_index=np.zeros(0, I32), face_building=np.zeros(0, I32)), **kw))


def _outlines(**kw):
    return NS(**dict(dict(n_labels=1, n_rings=0, n_vertices=0, n_half=0, ring_label=np.zeros(0, I32),
                          ring_start=np.zeros(0, I32), ring_length=np.zeros(0, I64), ring_vertices=np.zeros(0, I64),
                          ring_area2=np.zeros(0, I64), ring_bbox=np.zeros((0, 4), I32), ring_offset=np.zeros(1, I64),
                          label_ring_offset=np.zeros(2, I64), xy=np.zeros((0, 2), I32), z=None), **kw))


def _simple(**kw):
    return NS(**dict(dict(n_labels=1, n_rings=0, n_svertices=0, tol_num=0, tol_den=1, repair_rounds=0, n_forced=0,
                          ring_label=np.zeros(0, I32), ring_area2=np.zeros(0, I64), s_ring_offset=np.zeros(1, I64),
                          label_ring_offset=np.zeros(2, I64), sxy=np.zeros((0, 2), I32), sz=None), **kw))


def _triangles(**kw):
    return NS(**dict(dict(n_labels=1, n_svertices=0, n_triangles=0, n_failed_labels=0, n_bridges=0,
                          tri_offset=np.zeros(2, I64), label_status=np.zeros(1, I32), tri=np.zeros((0, 3), I32)), **kw))


def _buildings(**kw):
    b = api.Buildings(0, 4, 3, np.zeros((0, 2), I32), np.zeros((0, 4), I32), *[np.zeros(0, I64) for _ in range(4)],
                      np.zeros(0, I32), np.zeros(0, I32), np.zeros(0, I64))
    b.__dict__.update(kw)
    return b


def _roofs(**kw):
    return NS(**dict(dict(roof=LABEL, n_planes=0, normal=np.zeros((0, 3)), center=np.zeros((0, 3), I32), pixels=np.zeros(0, I64),
                          z_min=np.zeros(0, I32), z_max=np.zeros(0, I32), bin=100), **kw))


FP = NS(contours=[], area=np.zeros(0), perimeter=np.zeros(0), width=4, height=3)
NO_FACET, NO_TOP = _facets(facet=None), _solids(top=None)


def _cases():
    """(method, case, argument the message names, callable of a bare context)"""
    out = []
    add = lambda m, c, a, fn: out.append((m, c, a, fn))  # noqa: E731
    chain = {"facet_outlines": (), "simplified_outlines": (), "clean_outlines": (), "outline_triangles": (),
             "poly_solids": (SHORT[:1],), "model_raster": (), "point_residuals": (XYZ,)}
    for m, more in chain.items():
        add(m, "label 1-D", "label", lambda c, m=m, more=more: getattr(c, m)(FLAT_LABEL, TOP, *more))
        add(m, "top of the wrong shape", "top", lambda c, m=m, more=more: getattr(c, m)(LABEL, BAD_TOP, *more))
    for m in ("poly_solids", "model_raster", "point_residuals"):
        add(m, "top missing", "top", lambda c, m=m: getattr(c, m)(LABEL, None, *chain[m]))
    add("poly_solids", "label_building of the wrong length", "label_building", lambda c: c.poly_solids(LABEL, TOP, SHORT))
    add("knn_normals", "xyz [n][2]", "xyz", lambda c: c.knn_normals(XY2, api.Params()))
    add("assign_buildings", "xyz [n][2]", "xyz", lambda c: c.assign_buildings(XY2, BMAP, _buildings()))
    add("roofs", "xyz [n][2]", "xyz", lambda c: c.roofs(XY2, BMAP, PIDX, [], [], []))
    add("roofs", "bmap 1-D", "bmap", lambda c: c.roofs(XYZ, FLAT_LABEL, PIDX, [], [], []))
    add("roofs", "plane_idx of the wrong length", "plane_idx", lambda c: c.roofs(XYZ, BMAP, SHORT, [], [], []))
    add("plane_fit", "xyz [n][2]", "xyz", lambda c: c.plane_fit(XY2, PIDX, 1))
    add("plane_fit", "plane_idx of the wrong length", "plane_idx", lambda c: c.plane_fit(XYZ, SHORT, 1))
    add("point_residuals", "xyz [n][2]", "xyz", lambda c: c.point_residuals(LABEL, TOP, XY2))
    add("point_residuals", "plane_idx of the wrong length", "plane_idx",
        lambda c: c.point_residuals(LABEL, TOP, XYZ, n_labels=1, plane_idx=SHORT, label_plane=[0]))
    add("point_residuals", "clip2 not whole", "clip2", lambda c: c.point_residuals(LABEL, TOP, XYZ, clip2=1.5))
    add("terrain", "xyz [n][2]", "xyz", lambda c: c.terrain(XY2, BMAP, 1))
    add("terrain", "bmap 1-D", "bmap", lambda c: c.terrain(XYZ, FLAT_LABEL, 1))
    add("terrain", "q=(3, 2)", "q", lambda c: c.terrain(XYZ, BMAP, 1, q=(3, 2)))
    add("ground", "xyz [n][2]", "xyz", lambda c: c.ground(XY2))
    add("roof_evidence", "xyz [n][2]", "xyz", lambda c: c.roof_evidence(XY2, PIDX, 1))
    add("roof_evidence", "plane_idx of the wrong length", "plane_idx", lambda c: c.roof_evidence(XYZ, SHORT, 1))
    add("roof_evidence", "plane_ok of the wrong length", "plane_ok", lambda c: c.roof_evidence(XYZ, PIDX, 1, plane_ok=[1, 1]))
    add("footprints", "image 2-D", "image", lambda c: c.footprints(BMAP))
    add("building_map", "mask 1-D", "mask", lambda c: c.building_map(FLAT_LABEL))
    add("plane_buildings", "building_idx of the wrong length", "building_idx", lambda c: c.plane_buildings(PIDX, SHORT, 1, 1))
    add("solids", "roof image on the device", "roof", lambda c: c.solids(BMAP, _roofs(roof=None), base_z=0, flat=[]))
    add("solids", "bmap 1-D", "bmap", lambda c: c.solids(FLAT_LABEL, _roofs(), base_z=0, flat=[]))
    add("generalise_roofs", "roof image on the device", "roof",
        lambda c: c.generalise_roofs(BMAP, _roofs(roof=None), base_z=0, flat=[]))
    add("roof_facets", "top of the wrong shape", "top", lambda c: c.roof_facets(BMAP, LABEL, BAD_TOP))
    add("roof_structure", "roof image on the device", "roof", lambda c: c.roof_structure(BMAP, _roofs(roof=None), _solids()))
    add("roof_structure", "Solids without top", "top", lambda c: c.roof_structure(BMAP, _roofs(), NO_TOP))
    for m in ("roof_outlines", "roof_polygons", "roof_mesh", "building_model", "model_fidelity"):
        add(m, "roof_facets with facet=None", "facet", lambda c, m=m: getattr(c, m)(NO_FACET, _solids()))
        add(m, "Solids without top", "top", lambda c, m=m: getattr(c, m)(_facets(), NO_TOP))
    add("point_fidelity", "roof_facets with facet=None", "facet", lambda c: c.point_fidelity(XYZ, NO_FACET, _solids()))
    add("point_fidelity", "Solids without top", "top", lambda c: c.point_fidelity(XYZ, _facets(), NO_TOP))
    # the module-level writers: a bad origin, and dataclasses whose arrays do not fit their totals
    writers = {"write_buildings_obj": lambda **k: api.write_buildings_obj(FP, _buildings(), "x.obj", **k),
               "write_roofs_obj": lambda **k: api.write_roofs_obj(_roofs(), BMAP, "x.obj", **k),
               "write_solids_obj": lambda **k: api.write_solids_obj(_solids(), "x.obj", **k),
               "write_roof_edges_obj": lambda **k: api.write_roof_edges_obj(_facets(), BMAP, TOP, "x.obj", 100,
                                                                            kinds=np.zeros(0, np.uint8), **k),
               "write_outlines_obj": lambda **k: api.write_outlines_obj(_outlines(), "x.obj", 100, **k),
               "write_simple_outlines_obj": lambda **k: api.write_simple_outlines_obj(_simple(), "x.obj", 100, **k),
               "write_clean_outlines_obj": lambda **k: api.write_clean_outlines_obj(_simple(), "x.obj", 100, **k),
               "write_outline_triangles_obj": lambda **k: api.write_outline_triangles_obj(_triangles(), _simple(), "x.obj",
                                                                                          100, **k)}
    for m, fn in writers.items():
        add(m, "origin [2]", "origin", lambda c, fn=fn: fn(origin=BAD_ORIGIN))
    two = np.zeros(2, I64)
    add("write_buildings_obj", "pixels longer than n_buildings", "pixels",
        lambda c: api.write_buildings_obj(FP, _buildings(pixels=two), "x.obj"))
    add("write_buildings_obj", "area longer than the contours", "area",
        lambda c: api.write_buildings_obj(NS(**dict(FP.__dict__, area=np.zeros(2))), _buildings(), "x.obj"))
    add("write_roofs_obj", "pixels longer than n_planes", "pixels",
        lambda c: api.write_roofs_obj(_roofs(pixels=two), BMAP, "x.obj"))
    add("write_roofs_obj", "normal longer than n_planes", "normal",
        lambda c: api.write_roofs_obj(_roofs(normal=np.zeros((2, 3))), BMAP, "x.obj"))
    add("write_solids_obj", "face_offset longer than n_faces + 1", "face_offset",
        lambda c: api.write_solids_obj(_solids(face_offset=np.zeros(2, I32)), "x.obj"))
    add("write_solids_obj", "mesh on the device", "mesh", lambda c: api.write_solids_obj(_solids(vertex=None), "x.obj"))
    add("write_roof_edges_obj", "facet image on the device", "facet",
        lambda c: api.write_roof_edges_obj(NO_FACET, BMAP, TOP, "x.obj", 100))
    add("write_roof_edges_obj", "facet_building longer than n_facets", "facet_building",
        lambda c: api.write_roof_edges_obj(_facets(facet_building=np.zeros(2, I32)), BMAP, TOP, "x.obj", 100))
    add("write_roof_edges_obj", "kinds longer than n_edges", "kinds",
        lambda c: api.write_roof_edges_obj(_facets(), BMAP, TOP, "x.obj", 100, kinds=[0, 0]))
    add("roof_edge_kinds", "edge_length longer than n_edges", "edge_length",
        lambda c: api.roof_edge_kinds(_facets(edge_length=two)))
    add("write_outlines_obj", "ring_offset longer than n_rings + 1", "ring_offset",
        lambda c: api.write_outlines_obj(_outlines(ring_offset=two), "x.obj", 100))
    add("write_outlines_obj", "z longer than n_vertices", "z",
        lambda c: api.write_outlines_obj(_outlines(z=np.zeros(2, I32)), "x.obj", 100))
    add("write_outlines_obj", "vertices on the device", "vertices",
        lambda c: api.write_outlines_obj(_outlines(xy=None), "x.obj", 100))
    for m in ("write_simple_outlines_obj", "write_clean_outlines_obj"):
        add(m, "s_ring_offset longer than n_rings + 1", "s_ring_offset",
            lambda c, m=m: getattr(api, m)(_simple(s_ring_offset=two), "x.obj", 100))
        add(m, "sz longer than n_svertices", "sz", lambda c, m=m: getattr(api, m)(_simple(sz=np.zeros(2, I32)), "x.obj", 100))
    add("write_outline_triangles_obj", "tri_offset shorter than n_labels + 1", "tri_offset",
        lambda c: api.write_outline_triangles_obj(_triangles(tri_offset=np.zeros(1, I64)), _simple(), "x.obj", 100))
    add("write_outline_triangles_obj", "sxy longer than n_svertices", "sxy",
        lambda c: api.write_outline_triangles_obj(_triangles(), _simple(sxy=np.zeros((2, 2), I32)), "x.obj", 100))
    add("plane_fit_apply", "normal longer than n_planes", "normal",
        lambda c: api.plane_fit_apply(NS(n_planes=0), np.zeros((2, 3)), np.zeros((0, 3))))
    return out


def run_cases():
    """[{method, case, argument, type, names_method, message}] of every case of _cases(), on a bare context"""
    rows = []
    load = api._lib.load
    api._lib.load = lambda: _NoLibrary()
    try:
        for method, case, arg, fn in _cases():
            try:
                fn(bare_context())
                typ, msg = None, ""
            except Exception as e:  # noqa: BLE001 -- the type is what is recorded
                typ, msg = type(e).__name__, str(e)
            rows.append({"method": method, "case": case, "argument": arg, "type": typ, "names_method": method in msg,
                         "message": msg})
    finally:
        api._lib.load = load
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    surf = surface()
    rej = [{k: r[k] for k in ("method", "case", "argument", "type", "names_method")} for r in run_cases()]
    bad = [r for r in run_cases() if r["type"] in (None, "ReachedLibrary", "AttributeError") or r["argument"] not in r["message"]]
    for r in bad:
        print("NOT A RECORDABLE REJECT:", r)
    if a.write and not bad:
        row = lambda v: json.dumps(v, sort_keys=True)  # noqa: E731 -- one entry per line
        with open(os.path.join(DATA, "api_surface.json"), "w") as f:
            parts = [f"{row(part)}: {{\n" + ",\n".join(f" {row(k)}: {row(v)}" for k, v in sorted(d.items())) + "\n}"
                     for part, d in sorted(surf.items())]
            f.write("{\n" + ",\n".join(parts) + "\n}\n")
        with open(os.path.join(DATA, "api_rejects.json"), "w") as f:
            f.write("[\n" + ",\n".join(row(r) for r in rej) + "\n]\n")
    print(f"{len(surf['names'])} names, {len(surf['context'])} methods, {len(surf['dataclasses'])} dataclasses, {len(rej)} rejects")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
