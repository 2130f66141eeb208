"""Facet outlines without a GPU (include/bs_api.h, "facet outlines"): the numpy restatement of the device algorithm against
the brute force that walks every ring, the identities every result must satisfy, an even-odd check of the rings against the
label image, the regimes the device suite's cases reach, and the host-only writer bs_outlines_write_obj through the library
against the brute force's OBJ bytes."""
import ctypes as C
import importlib.util
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_facet_outlines_count_dev", "bs_facet_outlines_emit_dev", "bs_facet_outlines", "bs_outlines_free",
       "bs_outlines_write_obj"]
ORIGIN = (431200, -5620000, 87000)


def load_outline_cases():
    """tests/outline_ref/cases.py under a name of its own (other reference directories have a cases.py too)"""
    if "outline_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("outline_cases", os.path.join(HERE, "outline_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["outline_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["outline_cases"]


cases = load_outline_cases()
orf, brute, fc = cases.orf, cases.brute, cases.fc
NAMED = dict(cases.named_cases())


def even_odd(c, o):
    """pixel (x, y) has label l iff the even-odd count of l's rings around its centre is odd: a ray from the centre towards
    -x crosses the vertical edges between consecutive ring vertices at X <= x whose rows hold y"""
    label = np.asarray(c["label"])
    for l in range(o.n_labels):
        parity = np.zeros(label.shape, bool)
        for r in range(int(o.label_ring_offset[l]), int(o.label_ring_offset[l + 1])):
            pts = o.xy[o.ring_offset[r]:o.ring_offset[r + 1]].astype(np.int64)
            nxt = np.roll(pts, -1, axis=0)
            assert ((pts[:, 0] == nxt[:, 0]) ^ (pts[:, 1] == nxt[:, 1])).all()  # axis-parallel edges of non-zero length
            for (xa, ya), (xb, yb) in zip(pts, nxt):
                if xa == xb:
                    parity[min(ya, yb):max(ya, yb), xa:] ^= True
        assert np.array_equal(parity, label == l), l


def facet_identity(c, o):
    """(*) with the facet image: the half-edges of facet f are its inner and outer pixel edges"""
    f = c["facets"]
    per = np.zeros(o.n_labels, np.int64)
    np.add.at(per, o.ring_label, o.ring_length)
    assert np.array_equal(per, f.facet_inner_edges + f.facet_outer_edges)
    start = f.facet_start_xy[:, 1].astype(np.int64) * c["label"].shape[1] + f.facet_start_xy[:, 0]
    first = o.label_ring_offset[:-1]
    assert np.array_equal(o.ring_start[first], 4 * start)


def check_case(c, small, tmp_path=None):
    a, b = cases.run_ref(c), brute.outlines(c["label"], c["top"], c["n_labels"])
    assert orf.same(a, b) is None, orf.same(a, b)
    orf.identities(a, c["label"], c["connected"])
    if c["facets"] is not None:
        facet_identity(c, a)
    if small:
        even_odd(c, a)
    flat = orf.outlines(c["label"], None, c["n_labels"])  # without top: the same rings, no z
    assert flat.z is None and orf.same(flat, brute.outlines(c["label"], None, c["n_labels"])) is None
    assert np.array_equal(flat.xy, a.xy)
    if tmp_path is not None:
        for o in (a, flat):
            api.write_outlines_obj(o, tmp_path / "o.obj", 25, origin=ORIGIN)
            assert open(tmp_path / "o.obj", "rb").read() == brute.obj_text(o, 25, ORIGIN)
    return a


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert re.search(r"^struct bs_outlines \{", txt, flags=re.M)
    assert re.search(r"^#define BS_API_VERSION 5$", txt, flags=re.M)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.bs_api_version() == 5 == _lib.API_VERSION
    for name in ("facet_outlines", "facet_outlines_dev", "facet_outlines_emit_dev", "roof_outlines"):
        assert hasattr(api.Context, name), name
    for name in ("write_outlines_obj", "Outlines"):
        assert hasattr(api, name), name
    s = _lib.Outlines()
    L.bs_outlines_free(C.byref(s))  # a zeroed struct is accepted
    L.bs_outlines_free(None)


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case(name, tmp_path):
    c = NAMED[name]
    a = check_case(c, True, tmp_path)
    reg = cases.regimes(c, a)
    if name == "one_pixel":
        assert (a.n_half, a.n_rings, a.xy.tolist()) == (4, 1, [[0, 0], [1, 0], [1, 1], [0, 1]]) and "ring_of_4" in reg
    elif name == "plane_checkerboard":
        assert a.n_rings == 64 and (a.ring_length == 4).all() and "every_pixel_a_ring" in reg
    elif name == "ring_with_hole":
        assert a.ring_label.tolist() == [0, 0, 1] and a.ring_area2.tolist() == [50, -2, 2] and "label_in_hole" in reg
    elif name == "wide_hole":
        assert a.ring_start.tolist() == [0, 4 * (1 * 6 + 2) + 2] and a.ring_length.tolist() == [22, 6]
        assert a.xy[4:].tolist() == [[2, 2], [2, 3], [4, 3], [4, 2]] and "start_not_a_vertex" in reg
    elif name == "corner_twice":
        assert a.n_rings == 1 and a.xy.tolist().count([1, 2]) == 2 and "corner_twice" in reg
    elif name == "hole_touches_outer":
        assert a.n_rings == 1 and a.xy.tolist().count([1, 1]) == 2 and "hole_touches_outer" in reg
    elif name == "label_in_hole":
        assert a.ring_label.tolist() == [0, 0, 1] and "label_in_hole" in reg
    elif name == "two_holes":
        assert a.label_ring_offset.tolist() == [0, 3] and (a.ring_area2 > 0).tolist() == [True, False, False] and "three_rings" in reg
    elif name == "strip_31":
        assert (a.n_half, a.n_rings, a.n_vertices) == (64, 1, 4) and "n_half_power_of_two" in reg
    elif name == "strip_32":
        assert (a.n_half, a.n_rings, a.n_vertices) == (66, 1, 4) and "n_half_power_of_two_plus_2" in reg
    elif name == "full_image":
        assert a.ring_bbox.tolist() == [[0, 0, 9, 7]] and "border_all_sides" in reg
    elif name == "nothing":
        assert (a.n_half, a.n_rings, a.n_vertices) == (0, 0, 0) and a.ring_offset.tolist() == [0] and reg == {"no_pixel"}
        assert a.label_ring_offset.tolist() == [0]


@pytest.mark.parametrize("seed", range(fc.N_SOLID_FUZZ))
def test_solid_fuzz(seed, tmp_path):
    c = cases.from_facet(fc.solid_fuzz_case(seed))
    check_case(c, c["label"].size <= 4096, tmp_path)


@pytest.mark.parametrize("seed", range(fc.N_FUZZ))
def test_facet_fuzz(seed):
    check_case(cases.from_facet(fc.fuzz_case(seed)), False)


@pytest.mark.parametrize("seed", range(cases.N_RANDOM))
def test_random_labels(seed, tmp_path):
    c = cases.random_case(seed)
    assert max(c["label"].shape) <= 12 and not c["connected"]
    check_case(c, True, tmp_path)


@pytest.mark.parametrize("w,h", cases.LINE_SIZES)
def test_line_images(w, h):
    check_case(cases.line_case(w, h), True)


def test_cases_reach_every_regime():
    """Every row of the threshold table of DESIGN.md ("Facet outlines") is reached by the cases of
    tests/test_gpu_outlines.py: the named cases, the solid fuzz cases, the facet fuzz cases and the serpentine."""
    seen = Counter()
    for name, c in cases.all_cases():
        seen.update(cases.regimes(c))
    missing = [k for k in cases.REGIMES if seen[k] == 0]
    assert not missing, missing
    assert (fc.solid_fuzz_case(15)["bmap"] < 0).all()  # the case without a labelled pixel


def test_round_count_is_tight():
    """R = ceil(log2 n_half) rounds find the leader of a single ring of n_half half-edges; one round fewer does not reach
    around the 66 half-edges of the 32 x 1 strip"""
    for n, want in ((31, 6), (32, 7)):
        t = {}
        o = orf.outlines(np.zeros((1, n), np.int32), trace=t)
        assert o.n_half == 2 * n + 2 and t["R"] == want == orf.rounds_of(o.n_half) and (t["leader"] == 0).all()
    succ = t["succ"]
    mn, nxt = np.arange(66), succ.copy()
    for _ in range(6):
        mn, nxt = np.minimum(mn, mn[nxt]), nxt[nxt]
    assert (mn != 0).any()


def test_writer_error_paths(tmp_path):
    L = _lib.load()
    o = cases.run_ref(NAMED["wide_hole"])
    st, keep = api._outlines_struct(o)
    path = str(tmp_path / "x.obj").encode()
    assert L.bs_outlines_write_obj(C.byref(st), 10, None, path) == 0
    assert open(path, "rb").read() == brute.obj_text(o, 10)
    assert L.bs_outlines_write_obj(None, 10, None, path) == -1
    assert L.bs_outlines_write_obj(C.byref(st), 10, None, None) == -1
    assert L.bs_outlines_write_obj(C.byref(st), 0, None, path) == -1
    assert L.bs_outlines_write_obj(C.byref(st), 10, None, str(tmp_path / "no_such_dir" / "x.obj").encode()) == -1
    with pytest.raises(api.BsError):
        api.write_outlines_obj(o, tmp_path / "x.obj", 0)
    empty = cases.run_ref(NAMED["nothing"])
    api.write_outlines_obj(empty, tmp_path / "e.obj", 10)
    assert open(tmp_path / "e.obj", "rb").read() == b"# facet outlines: 0 labels, 0 rings, 0 vertices\n"
