"""Roof facets without a GPU (include/bs_api.h, "roof facets"): the numpy restatement against the per-pixel brute force,
the identities every result must satisfy, the regimes the device suite's cases reach, and the two host-only entry points
(bs_roof_edge_kinds, bs_roof_edges_write_obj) through the library against the reference's kinds and OBJ bytes."""
import ctypes as C
import importlib.util
import os
import sys
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def load_facet_cases():
    """tests/facet_ref/cases.py and brute.py under names of their own (other reference directories have the same)"""
    return _load("facet_cases", os.path.join(HERE, "facet_ref", "cases.py"))


cases = load_facet_cases()
fr = cases.fr
fbrute = fr.brute
sr = cases.sr

NEW = ["bs_roof_facets_dev", "bs_roof_facets", "bs_roof_facets_free", "bs_roof_edge_kinds", "bs_roof_edges_write_obj"]
SHAPES = cases.named_shapes()
ORIGIN = (431200, -5620000, 87000)


def identities(c, r):
    """what every result satisfies, from the inputs and the arrays alone"""
    bmap, top = np.asarray(c["bmap"], np.int64), np.asarray(c["top"], np.int64)
    inb = bmap >= 0
    assert r.n_pixels == int(inb.sum()) == int(r.facet_pixels.sum())
    assert (r.facet >= 0).sum() == r.n_pixels and ((r.facet < 0) == ~inb).all()
    facet = r.facet.astype(np.int64)
    # 4 * pixels = 2 * (neighbour pairs inside the facet) + inner_edges + outer_edges, per facet
    pairs = np.zeros(r.n_facets, np.int64)
    for a, b in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                 ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        inside = (facet[a] >= 0) & (facet[a] == facet[b])
        np.add.at(pairs, facet[a][inside], 1)
    assert np.array_equal(4 * r.facet_pixels, 2 * pairs + r.facet_inner_edges + r.facet_outer_edges)
    assert int(r.facet_inner_edges.sum()) == 2 * r.n_border == 2 * int(r.edge_length.sum())
    # n_step: the same-building pixel edges whose tops differ, counted directly from top
    direct = 0
    for a, b, ka, kb in (((slice(None), slice(None, -1)), (slice(None), slice(1, None)), (1, 3), (0, 2)),
                         ((slice(None, -1), slice(None)), (slice(1, None), slice(None)), (2, 3), (0, 1))):
        same_b = (bmap[a] >= 0) & (bmap[a] == bmap[b])
        differ = (top[a][..., ka[0]] != top[b][..., kb[0]]) | (top[a][..., ka[1]] != top[b][..., kb[1]])
        direct += int((same_b & differ).sum())  # (inside a facet the tops at a shared corner are one number)
    assert int(r.edge_n_step.sum()) == direct
    if r.n_edges:
        assert (r.edge_facet[:, 0] < r.edge_facet[:, 1]).all()
        key = r.edge_facet[:, 0].astype(np.int64) * r.n_facets + r.edge_facet[:, 1]
        assert (np.diff(key) > 0).all()
        assert np.array_equal(r.edge_building, r.facet_building[r.edge_facet[:, 0]])
        assert np.array_equal(r.edge_building, r.facet_building[r.edge_facet[:, 1]])
    if r.n_facets:
        start = r.facet_start_xy[:, 1].astype(np.int64) * bmap.shape[1] + r.facet_start_xy[:, 0]
        assert (np.diff(start) > 0).all()  # ascending start pixel


def outer_walls(c, r):
    """the outer edges of the image whose tops are not both base_z: where the solids put an outer wall"""
    bmap, top, base = np.asarray(c["bmap"], np.int64), np.asarray(c["top"], np.int64), c["solid"]["base_z"]
    h, w = bmap.shape
    pm = np.full((h + 2, w + 2), -2, np.int64)
    pm[1:-1, 1:-1] = np.where(bmap >= 0, bmap, -1)
    ys, xs = np.nonzero(bmap >= 0)
    n = 0
    for (dx, dy), (ks, ke) in (((0, -1), (0, 1)), ((1, 0), (1, 3)), ((0, 1), (3, 2)), ((-1, 0), (2, 0))):
        outer = pm[ys + 1 + dy, xs + 1 + dx] != bmap[ys, xs]
        n += int((outer & ((top[ys, xs, ks] != base) | (top[ys, xs, ke] != base))).sum())
    return n


def solids_cross_check(c, r, n_wall_faces):
    """the solids' walls = the inner steps + the outer edges that stand above base_z"""
    assert n_wall_faces == int(r.edge_n_step.sum()) + outer_walls(c, r)


def lib_kinds(r, step_tol, bend_tol):
    return api.roof_edge_kinds(r, step_tol, bend_tol)


def check_host_entry_points(c, r, tmp_path):
    """bs_roof_edge_kinds and bs_roof_edges_write_obj through the library against the reference"""
    for tols in (cases.KIND_TOLS, (200, 0), (0, 0), (5, 30)):
        want = fr.kinds(r, *tols)
        assert np.array_equal(lib_kinds(r, *tols), want), tols
        assert np.array_equal(fbrute.kinds(r, *tols), want), tols
    kind = fr.kinds(r, *cases.KIND_TOLS)
    path = str(tmp_path / "edges.obj")
    api.write_roof_edges_obj(r, c["bmap"], c["top"], path, c["bin"], kinds=kind, origin=ORIGIN)
    data = open(path, "rb").read()
    assert data == fr.obj_text(r, c["bmap"], c["top"], c["bin"], kind, ORIGIN)
    assert data.startswith(f"# roof edges: {r.n_edges} edges, {r.n_border} segments\n".encode())
    return data


def test_symbols_and_python_names():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.bs_api_version() == 5
    for name in ("roof_facets", "roof_facets_dev", "roof_structure"):
        assert hasattr(api.Context, name), name
    for name in ("roof_edge_kinds", "write_roof_edges_obj", "RoofFacets"):
        assert hasattr(api, name), name
    s = _lib.RoofFacets()
    L.bs_roof_facets_free(C.byref(s))  # a zeroed struct is accepted
    L.bs_roof_facets_free(None)


@pytest.mark.parametrize("seed", range(cases.N_SMALL))
def test_restatement_equals_brute_force(seed, tmp_path):
    c = cases.small_case(seed)
    assert max(c["bmap"].shape) <= 12
    a, b = cases.run_ref(c), fbrute.roof_facets(c["bmap"], c["roof"], c["top"])
    assert fr.same(a, b) is None, fr.same(a, b)
    identities(c, a)
    solids_cross_check(c, a, cases.sc.run_ref(c["solid"]).n_wall_faces)
    kind = fr.kinds(a, *cases.KIND_TOLS)
    assert fbrute.obj_text(a, c["bmap"], c["top"], c["bin"], kind, ORIGIN) == fr.obj_text(a, c["bmap"], c["top"], c["bin"], kind,
                                                                                         ORIGIN)
    check_host_entry_points(c, a, tmp_path)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_named_shape(name, tmp_path):
    c = SHAPES[name]
    a, b = cases.run_ref(c), fbrute.roof_facets(c["bmap"], c["roof"], c["top"])
    assert fr.same(a, b) is None, fr.same(a, b)
    identities(c, a)
    solids_cross_check(c, a, cases.sc.run_ref(c["solid"]).n_wall_faces)
    check_host_entry_points(c, a, tmp_path)
    reg = cases.regimes(c, a)
    kinds = fr.kinds(a, 200, 0).tolist()
    if name == "one_pixel":
        assert (a.n_facets, a.n_edges, a.facet_outer_edges.tolist()) == (1, 0, [4])
    elif name == "two_pixels_one_plane":
        assert (a.n_facets, a.n_edges, a.facet_pixels.tolist(), a.facet_outer_edges.tolist()) == (1, 0, [2], [6])
    elif name == "two_pixels_diagonal":
        assert (a.n_facets, a.n_edges) == (2, 0) and a.facet.tolist() == [[0, -1], [-1, 1]]
    elif name == "two_buildings_same_plane":
        assert (a.n_facets, a.n_edges, a.facet_outer_edges.tolist()) == (2, 0, [4, 4]) and "other_building_same_plane" in reg
    elif name == "ring_with_hole":
        assert (a.n_facets, a.n_edges, a.edge_length.tolist()) == (2, 1, [4]) and "facet_with_hole" in reg
        assert "edge_both_directions" in reg and a.edge_bbox.tolist() == [[2, 2, 3, 3]]
    elif name == "serpentine":
        assert a.facet_pixels[0] == 20 * 130 + 20 and a.n_facets == 1 + 20 and "facet_spans_tiles_x" in reg
        assert "facet_spans_tiles_y" in reg and "tile_local_split" in reg
    elif name in ("comb_x", "comb_y"):
        assert a.facet_plane[0] == 1 and a.facet_start_xy[0].tolist() == [0, 0] and "tile_local_split" in reg
        assert ("facet_spans_tiles_x" if name == "comb_x" else "facet_spans_tiles_y") in reg
        assert (a.facet_plane == 1).sum() == 1  # all teeth are one facet
    elif name == "same_plane_two_pieces":
        assert a.facet.tolist() == [[0, 1, 2]] and a.edge_facet.tolist() == [[0, 1], [1, 2]] and "same_plane_two_facets" in reg
    elif name == "two_flat_planes_equal_height":
        assert a.edge_n_step.tolist() == [0] and a.edge_length.tolist() == [2] and kinds == [0] and "edge_no_step" in reg
    elif name == "gable":
        assert a.edge_n_step.tolist() == [0] and a.edge_bend_sum.tolist() == [3 * 40] and kinds == [1]
    elif name == "inverted_gable":
        assert a.edge_n_step.tolist() == [0] and a.edge_bend_sum.tolist() == [-3 * 40] and kinds == [2]
    elif name == "plane_checkerboard":
        assert a.n_facets == 64 and a.n_edges == 2 * 8 * 7 and (a.facet_pixels == 1).all() and set(kinds) == {3}
        assert "diagonal_contact" in reg and "many_facets" in reg


def test_cases_reach_every_regime():
    """Every row of the threshold table of DESIGN.md ("Roof facets") is reached by the cases of tests/test_gpu_facets.py:
    the named shapes, the solid fuzz cases and the facet fuzz cases."""
    seen = Counter()
    for name, c in cases.all_cases():
        seen.update(cases.regimes(c))
    missing = [k for k in cases.REGIMES if seen[k] == 0]
    assert not missing, missing
    assert set(seen) <= set(cases.REGIMES)


@pytest.mark.parametrize("seed", range(cases.N_SOLID_FUZZ))
def test_solid_fuzz_identities_and_host_entry_points(seed, tmp_path):
    c = cases.solid_fuzz_case(seed)
    r = cases.run_ref(c)
    identities(c, r)
    solids_cross_check(c, r, cases.sc.run_ref(c["solid"]).n_wall_faces)
    check_host_entry_points(c, r, tmp_path)


@pytest.mark.parametrize("seed", range(cases.N_FUZZ))
def test_facet_fuzz_identities_and_host_entry_points(seed, tmp_path):
    c = cases.fuzz_case(seed)
    r = cases.run_ref(c)
    identities(c, r)
    check_host_entry_points(c, r, tmp_path)


def test_host_entry_point_error_paths(tmp_path):
    L = _lib.load()
    c = SHAPES["same_plane_two_pieces"]
    r = cases.run_ref(c)
    st, keep = api._roof_facets_struct(r)
    kind = np.zeros(2, np.uint8)
    assert L.bs_roof_edge_kinds(C.byref(st), 0, 0, kind.ctypes.data) == 0
    assert L.bs_roof_edge_kinds(None, 0, 0, kind.ctypes.data) == -1
    assert L.bs_roof_edge_kinds(C.byref(st), 0, 0, None) == -1
    assert L.bs_roof_edge_kinds(C.byref(st), -1, 0, kind.ctypes.data) == -1
    assert L.bs_roof_edge_kinds(C.byref(st), 0, -1, kind.ctypes.data) == -1
    with pytest.raises(api.BsError):
        api.roof_edge_kinds(r, step_tol=-5)
    facet, bmap, top = (np.ascontiguousarray(a, np.int32) for a in (r.facet, c["bmap"], c["top"]))
    path = str(tmp_path / "x.obj").encode()

    def call(facet=facet, bmap=bmap, top=top, bin=10, st=st, kind=kind, path=path):
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.bs_roof_edges_write_obj(p(facet), p(bmap), p(top), 3, 1, bin, None if st is None else C.byref(st), p(kind), None,
                                         path)

    assert call() == 0
    assert open(path, "rb").read() == fr.obj_text(r, bmap, top, 10, kind)
    assert call(facet=None) == -1 and call(bmap=None) == -1 and call(top=None) == -1 and call(st=None) == -1
    assert call(kind=None) == -1 and call(path=None) == -1 and call(bin=0) == -1
    assert call(path=str(tmp_path / "no_such_dir" / "x.obj").encode()) == -1
    other = np.array([[0, 2, 1]], np.int32)  # the pair (1, 2) exists, (0, 2) too, but a facet image with the pair (0, 3) not
    other[0, 1] = 3
    assert call(facet=other) == -1
    with pytest.raises(api.BsError):
        api.write_roof_edges_obj(r, bmap, top, tmp_path / "no_such_dir" / "x.obj", 10)
    # no building pixel: a header alone
    empty = SimpleNamespace(**{**vars(r), "n_facets": 0, "n_edges": 0, "n_pixels": 0, "n_border": 0,
                               "facet": np.full((1, 3), -1, np.int32)})
    for name, dt, cols in api._FACET_ARRAYS + api._EDGE_ARRAYS:
        setattr(empty, name, np.zeros((0, cols) if cols > 1 else (0,), dt))
    api.write_roof_edges_obj(empty, np.full((1, 3), -1), top, tmp_path / "e.obj", 10)
    assert open(tmp_path / "e.obj", "rb").read() == b"# roof edges: 0 edges, 0 segments\n"
