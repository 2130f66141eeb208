"""Outline triangles without a GPU (include/bs_api.h, "outline triangles"): the numpy restatement of the device algorithm
against the brute force of the definition on every run of the cases, and the identities every OK label must satisfy --
checked without the algorithm: the count, the orientation, the area, the pairing of directed edges, and on small images an
all-pairs test that no triangle edge crosses or touches the interior of a ring segment of its label."""
import importlib.util
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_outline_triangles_count_dev", "bs_outline_triangles_emit_dev", "bs_outline_triangles", "bs_outline_triangles_free",
       "bs_outline_triangles_write_obj"]


def load_triangulate_cases():
    if "triangulate_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("triangulate_cases", os.path.join(HERE, "triangulate_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["triangulate_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["triangulate_cases"]


cases = load_triangulate_cases()
tref, brute, uref = cases.tref, cases.brute, cases.uref
NAMED = dict(cases.uc.named_cases())
OWN = cases.own_shapes()
RUNS = {name: (c, cases.TOLERANCES) for name, c in NAMED.items()}
RUNS.update(OWN)
_REF = {}


def ref(name, tol):
    """(plain, clean, triangles) of the restatements, computed once and never changed"""
    if (name, tol) not in _REF:
        c = RUNS[name][0]
        plain, _, clean = uref.clean(c["label"], c["top"], c["n_labels"], *tol)
        _REF[name, tol] = (plain, clean, tref.triangulate(plain, clean))
    return _REF[name, tol]


def orient(P, a, b, c):
    return (P[b][0] - P[a][0]) * (P[c][1] - P[a][1]) - (P[b][1] - P[a][1]) * (P[c][0] - P[a][0])


def crossing_edges(P, edges, segments):
    """an all-pairs test of its own: the (edge, segment) pairs in which the triangle edge A-B and the ring segment C-D have
    a common point that is interior to C-D -- from the parameters of the common point as integers; collinear pairs count
    when they overlap in more than a point and are not the same segment"""
    e, g = np.array(edges, np.int64).reshape(-1, 4), np.array(segments, np.int64).reshape(-1, 4)
    a, c = np.repeat(e, len(g), axis=0), np.tile(g, (len(e), 1))
    rx, ry, sx, sy = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
    qx, qy = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
    den, un, vn = rx * sy - ry * sx, qx * sy - qy * sx, qx * ry - qy * rx
    sg = np.where(den < 0, -1, 1)
    den, un, vn = den * sg, un * sg, vn * sg
    meet = (den != 0) & (un >= 0) & (un <= den) & (vn >= 0) & (vn <= den)
    bad = meet & (vn > 0) & (vn < den)
    rr, t0 = rx * rx + ry * ry, qx * rx + qy * ry
    t1 = t0 + sx * rx + sy * ry
    lo, hi = np.maximum(np.minimum(t0, t1), 0), np.minimum(np.maximum(t0, t1), rr)
    same = (np.minimum(t0, t1) == 0) & (np.maximum(t0, t1) == rr)
    bad |= (den == 0) & (vn == 0) & (lo < hi) & ~same
    return int(bad.sum())


def check_identities(plain, clean, t, all_pairs):
    """the promises of include/bs_api.h for every OK label, none of them through the algorithm"""
    P = np.asarray(clean.sxy, np.int64).tolist()
    soff, lro = clean.s_ring_offset, plain.label_ring_offset
    for l in range(t.n_labels):
        r0, r1 = int(lro[l]), int(lro[l + 1])
        tri = t.tri[int(t.tri_offset[l]):int(t.tri_offset[l + 1])].tolist()
        if r0 == r1:
            assert t.label_status[l] == brute.EMPTY and not tri
            continue
        V = int(soff[r1] - soff[r0])
        O = int((np.asarray(plain.ring_area2[r0:r1]) > 0).sum())
        assert len(tri) == V + 2 * (r1 - r0 - O) - 2 * O
        if t.label_status[l] != brute.OK:
            assert (np.array(tri) == -1).all() and t.label_area2[l] == 0 and (t.bridge[r0:r1] == -1).all()
            continue
        assert all(orient(P, a, b, c) > 0 for a, b, c in tri)
        assert sum(orient(P, a, b, c) for a, b, c in tri) == t.label_area2[l] == int(np.asarray(clean.s_ring_area2[r0:r1]).sum())
        directed = Counter(e for a, b, c in tri for e in ((a, b), (b, c), (c, a)))
        assert set(directed.values()) == {1}
        ring_edges = set()
        for r in range(r0, r1):
            a, b = int(soff[r]), int(soff[r + 1])
            ring_edges |= {(v, v + 1 if v + 1 < b else a) for v in range(a, b)}
            hole = plain.ring_area2[r] <= 0
            assert (t.bridge[r, 0] >= 0) == hole and (not hole or (a <= t.bridge[r, 0] < b and not a <= t.bridge[r, 1] < b))
        assert ring_edges <= set(directed)
        inner = set(directed) - ring_edges
        assert all((b, a) in inner for a, b in inner)
        if all_pairs:
            edges = [P[a] + P[b] for a, b in inner if a < b]
            assert crossing_edges(P, edges, [P[a] + P[b] for a, b in ring_edges]) == 0 if edges else True


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert re.search(r"^struct bs_outline_triangles \{", txt, flags=re.M)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("outline_triangles", "outline_triangles_dev", "outline_triangles_emit_dev", "roof_mesh"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "OutlineTriangles") and hasattr(api, "write_outline_triangles_obj")
    assert L.bs_api_version() == 5
    caps = {k: int(v) for k, v in re.findall(r"^#define BS_TRI_(WAVE_CAP|LDS_CAP) (\d+)", txt, flags=re.M)}
    assert caps == {"WAVE_CAP": _lib.TRI_WAVE_CAP, "LDS_CAP": _lib.TRI_LDS_CAP} == {"WAVE_CAP": tref.WAVE_CAP, "LDS_CAP": tref.LDS_CAP}
    codes = {k: int(v) for k, v in re.findall(r"^#define (BS_TRI_[A-Z_]+) (\d)\b", txt, flags=re.M)}
    assert codes == {v: k for k, v in _lib.TRI_STATUS.items()}
    assert (brute.OK, brute.NO_BRIDGE, brute.STALLED, brute.EMPTY) == (0, 1, 2, 3)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_references_agree_and_identities_hold(name):
    """on every run of the cases: the restatement equals the definition in every array and total, and every OK label keeps
    the promises; the all-pairs test on the images up to 900 pixels"""
    c, tols = RUNS[name]
    for tol in tols:
        plain, clean, a = ref(name, tol)
        b = brute.triangulate(plain, clean)
        assert brute.same(a, b) is None, (tol, brute.same(a, b))
        check_identities(plain, clean, a, c["label"].size <= 900)


def test_statuses_of_the_named_runs():
    """a status other than OK must not hide a failure: of all named runs exactly one label is NO_BRIDGE, none is STALLED;
    every facet fuzz case and every shape is OK throughout"""
    failed = []
    for name, (c, tols) in RUNS.items():
        for tol in tols:
            _, _, t = ref(name, tol)
            failed += [(name, tol, l, int(s)) for l, s in enumerate(t.label_status) if s in (brute.NO_BRIDGE, brute.STALLED)]
    assert failed == [(n, tol, l, brute.NO_BRIDGE) for n, tol, l in cases.NO_BRIDGE_RUNS]
    assert all(n.startswith("random_") for n, _, _ in cases.NO_BRIDGE_RUNS)


def test_no_bridge_run_is_a_hole_outside_its_outer_ring():
    """random_0 at (10^6, 1), label 0: the chord (6, 0) -> (2, 8) of the outer ring sweeps over the whole hole ring (5, 6)
    (4, 6) (4, 7) (5, 7) without touching it; the clean outlines report no conflict, the triangles report NO_BRIDGE"""
    (name, tol, l), = cases.NO_BRIDGE_RUNS
    plain, clean, t = ref(name, tol)
    assert clean.n_marked_left == 0 and t.n_failed_labels == 1
    r0, r1 = int(plain.label_ring_offset[l]), int(plain.label_ring_offset[l + 1])
    rings = [clean.sxy[int(clean.s_ring_offset[r]):int(clean.s_ring_offset[r + 1])].tolist() for r in range(r0, r1)]
    hole = [[5, 6], [4, 6], [4, 7], [5, 7]]
    assert hole in rings and any([6, 0] in g and [2, 8] in g for g in rings)
    outer = next(g for g in rings if [6, 0] in g)
    i = outer.index([6, 0])
    assert outer[(i + 1) % len(outer)] == [2, 8]
    assert all((2 - 6) * (y - 0) - (8 - 0) * (x - 6) < 0 for x, y in hole)  # the whole hole on the right of the chord


def test_shapes_reach_what_they_are_for():
    r = {name: ref(name, (0, 1))[2] for name in OWN}
    comb = r["comb_300"]
    assert comb.n_triangles == 1202 and comb.max_label_occurrences == 1204 and comb.n_tests > 10 * comb.n_triangles
    assert r["long_comb"].max_label_occurrences > tref.LDS_CAP and r["long_comb"].n_labels_global == 1
    assert r["sieve_24"].n_labels_lds == 1 and r["sieve_30"].n_bridges == 49
    assert int((RUNS["sieve_24"][0]["label"] < 0).sum()) == 64
    t = {}
    plain, clean, _ = ref("blocked_nearest", (0, 1))
    tref.triangulate(plain, clean, t)
    assert t["blocked_candidates"] == 2
    plain, clean, e = ref("equal_left", (0, 1))
    m = clean.sxy[e.bridge[e.bridge[:, 0] >= 0][:, 0]]
    assert len(m) == 2 and m[0, 0] == m[1, 0]
    plain, clean, p = ref("pinched", (0, 1))
    assert clean.n_rings == 1 and len(set(map(tuple, clean.sxy.tolist()))) == clean.n_svertices - 1 and p.n_triangles == 8
    plain, _, two = ref("two_outers", (0, 1))
    assert (np.asarray(plain.ring_area2[:int(plain.label_ring_offset[1])]) > 0).sum() == 2 and two.n_bridges == 2
    assert r["nested"].n_bridges == 3 and (r["nested"].label_status == brute.OK).all()
    assert r["comb_300"].n_labels_global == 1 and r["nested"].n_labels_wave == 4


def test_obj_text_of_the_reference():
    plain, clean, t = ref("nested", (0, 1))
    text = brute.obj_text(t, clean, 25, (1000, -2000, 30)).decode()
    lines = text.split("\n")
    assert lines[0] == "# outline triangles: 4 labels, 28 vertices, 26 triangles, 0 failed labels, 3 bridges" and lines[-1] == ""
    assert sum(s.startswith("v ") for s in lines) == 28 and sum(s.startswith("f ") for s in lines) == 26
    assert [s for s in lines if s.startswith("g ")] == [f"g label_{l}" for l in range(4)]
    assert all(re.fullmatch(r"(v|f)( -?\d+){3}|g label_\d+|# .*|", s) for s in lines)
