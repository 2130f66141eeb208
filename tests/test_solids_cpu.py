"""Solids without a GPU (include/bs_api.h, "solids"): the numpy restatement against the per-pixel brute force, the two
properties that make the mesh a solid -- (a) every directed edge occurs as often as its reverse, (b) the determinant sum
of the fan triangles equals bin^2 * volume6 per building -- from the arrays and from the OBJ of bs_solids_write_obj
parsed back, the named shapes, the writer's error paths, and the regimes the device suite's fuzz cases reach."""
import ctypes as C
import importlib.util
import os
import sys
from collections import Counter

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "solid_ref"))
import brute  # noqa: E402
import solid_ref as sr  # noqa: E402


def load_solid_cases():
    """tests/solid_ref/cases.py under a name of its own (tests/fit_ref has a cases.py too)"""
    if "solid_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("solid_cases", os.path.join(HERE, "solid_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["solid_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["solid_cases"]


cases = load_solid_cases()

NEW = ["bs_solids_count_dev", "bs_solids_emit_dev", "bs_solids", "bs_solids_free", "bs_solids_write_obj"]


def check_solid(m, n_buildings, bin, volume6):
    """properties (a) and (b) of a mesh, from its arrays alone"""
    assert sr.unmatched_edges(m) == 0
    with np.errstate(over="ignore"):
        assert np.array_equal(sr.det_sums(m, n_buildings), np.int64(bin) ** 2 * np.asarray(volume6, np.int64))


def check_obj(m, c, path, origin=(431200, -5620000, 87000)):
    """the library's OBJ of mesh m equals the restatement's text, and the mesh parsed back from it is the same solid"""
    api.write_solids_obj(m, path, origin=origin)
    data = open(path, "rb").read()
    assert data == sr.obj_text(m, origin)
    back = sr.parse_obj(data)
    assert len(back.vertex) == m.n_vertices and len(back.face_building) == m.n_faces
    check_solid(back, c["n_buildings"], c["bin"], m.volume6)  # (a closed mesh: the shift by origin changes no sum)
    return data


def test_symbols_and_python_names():
    L = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.bs_api_version() == 5
    for name in ("solids", "solids_dev", "solids_emit_dev", "solid_model"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "write_solids_obj") and hasattr(api, "Solids")
    s = _lib.Solids()
    L.bs_solids_free(C.byref(s))  # a zeroed struct is accepted
    L.bs_solids_free(None)


@pytest.mark.parametrize("seed", range(cases.N_SMALL))
def test_restatement_equals_brute_force(seed, tmp_path):
    c = cases.small_case(seed)
    assert max(c["bmap"].shape) <= 12
    a, b = cases.run_ref(c), brute.solids(*[c[k] for k in cases.KEYS])
    assert sr.same(a, b) is None, sr.same(a, b)
    check_solid(a, c["n_buildings"], c["bin"], a.volume6)
    check_obj(a, c, str(tmp_path / "s.obj"))
    if a.n_faces:
        ln = np.diff(a.face_offset)
        assert ln.min() >= 3 and ln.max() <= 8 and (ln[a.face_kind == 0] == 3).all() and (ln[a.face_kind == 1] == 4).all()
    v = a.vertex.astype(np.int64)  # ascending (Y, X, c, Z), no vertex twice
    assert np.array_equal(np.lexsort((v[:, 2], v[:, 3], v[:, 0], v[:, 1])), np.arange(len(v)))
    assert len(np.unique(v, axis=0)) == len(v)


def test_small_cases_hold_what_they_are_for():
    seen = Counter()
    for seed in range(cases.N_SMALL):
        seen.update(cases.regimes(cases.small_case(seed)))
    for k in ("other_building", "unroofed", "top_at_base", "wall_inner", "wall_outer", "wall_mid_up", "wall_mid_down",
              "wall_crossing", "wall_triangle", "corner_8", "no_planes"):
        assert seen[k] > 0, k


SHAPES = cases.named_shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_named_shape(name, tmp_path):
    c = SHAPES[name]
    a, b = cases.run_ref(c), brute.solids(*[c[k] for k in cases.KEYS])
    assert sr.same(a, b) is None, sr.same(a, b)
    check_solid(a, c["n_buildings"], c["bin"], a.volume6)
    check_obj(a, c, str(tmp_path / "s.obj"))
    walls = sorted(np.diff(a.face_offset)[a.face_kind == 2].tolist())
    if name == "one_pixel":
        assert (a.n_vertices, a.n_faces, walls) == (8, 7, [4, 4, 4, 4]) and a.volume6.tolist() == [6 * 50]
    elif name == "one_pixel_at_base":
        assert (a.n_vertices, a.n_faces, walls) == (4, 3, []) and a.volume6.tolist() == [0]
    elif name == "two_pixels_triangle":
        assert walls.count(3) == 1 and a.n_crossing_walls == 0 and a.n_wall_faces == 7
    elif name == "two_pixels_quad":
        assert a.n_crossing_walls == 0 and a.n_wall_faces == 7 and 3 not in walls
        assert a.top[0, 0].tolist() == [100] * 4 and a.top[0, 1].tolist() == [120] * 4
    elif name == "two_pixels_crossing":
        assert a.crossing_walls.tolist() == [1] and a.top[0, 1].tolist() == [95, 95, 105, 105]
    elif name == "corner_four_heights":
        assert 5 in walls and 6 in walls and a.n_vertices == 4 * 3 + 4 * 2 + 5
    elif name == "checkerboard":
        assert a.n_pixels == 21 and a.n_faces == 3 * 21 + 4 * 21  # every pixel stands alone: four walls each
    elif name == "two_buildings":
        # each closed on its own (check_solid is per building) and nothing shared: a vertex belongs to one building
        assert (a.vertex[a.face_index, 3] == np.repeat(a.face_building, np.diff(a.face_offset))).all()
        assert a.faces.tolist() == [np.sum(a.face_building == 0), np.sum(a.face_building == 1)]
    elif name == "borders":
        assert a.n_pixels == 4 and a.n_wall_faces == 16


def test_writer_error_paths(tmp_path):
    L = _lib.load()
    a = cases.run_ref(SHAPES["two_buildings"])
    v, off, idx, fb = (np.ascontiguousarray(getattr(a, k)) for k in ("vertex", "face_offset", "face_index", "face_building"))
    path = str(tmp_path / "x.obj").encode()

    def call(v=v, nv=None, off=off, idx=idx, fb=fb, nf=None, nb=2, path=path):
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.bs_solids_write_obj(p(v), len(a.vertex) if nv is None else nv, p(off), p(idx), p(fb),
                                     len(a.face_building) if nf is None else nf, nb, None, path)

    assert call() == 0
    assert call(v=None) == -1 and call(off=None) == -1 and call(idx=None) == -1 and call(fb=None) == -1 and call(path=None) == -1
    assert call(nv=-1) == -1 and call(nf=-1) == -1 and call(nb=-1) == -1
    assert call(nb=1) == -1  # a face of building 1
    assert call(nv=len(a.vertex) - 1) == -1  # a vertex number out of range
    bad = off.copy()
    bad[0] = 1
    assert call(off=bad) == -1
    bad = off.copy()
    bad[3] = bad[2] - 1
    assert call(off=bad) == -1
    bad = idx.copy()
    bad[5] = -1
    assert call(idx=bad) == -1
    assert call(path=str(tmp_path / "no_such_dir" / "x.obj").encode()) == -1
    with pytest.raises(api.BsError):
        api.write_solids_obj(a, tmp_path / "no_such_dir" / "x.obj")
    # no vertex and no face: a header alone
    assert L.bs_solids_write_obj(None, 0, np.zeros(1, np.int32).ctypes.data, None, None, 0, 0, None, path) == 0
    assert open(path, "rb").read() == b"# solids: 0 buildings, 0 vertices, 0 faces\n"


def test_fuzz_cases_reach_every_regime():
    """Every row of the threshold table of DESIGN.md ("Solids") that an image of at most 96 x 96 can reach is reached by
    the fuzz cases of tests/test_gpu_solids.py (the grid strides and the scan's tiles are that file's large image)."""
    seen = Counter()
    for seed in range(cases.N_FUZZ):
        c = cases.fuzz_case(seed)
        assert max(c["bmap"].shape) <= 96
        seen.update(cases.regimes(c))
    missing = [k for k in cases.REGIMES if seen[k] == 0]
    assert not missing, missing
    assert set(seen) <= set(cases.REGIMES)
