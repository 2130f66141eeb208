"""Oriented boxes without a GPU (include/bs_api.h, "oriented boxes"): the definition in Python integers (tests/hull_ref/brute.py)
against scipy's qhull and against every pair direction, the identities of the header, the numpy restatement of the device pass
(tests/hull_ref/hull_ref.py) against the definition, and the host-only writer and corner rounding of the library against
Python."""
import ctypes as C
import functools
import importlib.util
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

from buildingsegment_amd import _lib, api, hulls

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def load_hull_cases():
    """tests/hull_ref/cases.py under a name of its own"""
    if "hull_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("hull_cases", os.path.join(HERE, "hull_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["hull_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["hull_cases"]


cases = load_hull_cases()
brute, ref = cases.brute, cases.ref
NAMED = dict(cases.named_cases())
FUZZ = dict(cases.fuzz_cases())
NEW = ("bs_label_hulls_count_dev", "bs_label_hulls_emit_dev", "bs_label_hulls", "bs_label_hulls_free", "bs_hull_box_corners",
       "bs_hull_boxes_write_obj")
# The issue lists the tie of the discs as edges 0, 0, 2, 7, 0.  By the definition (the list begins at the lowest corner index
# and runs with a positive shoelace sum, edge i leaves vertex i) the tied edges are 1, 1, 3, 8, 1: the issue's figures are the
# same edges counted from the list's second vertex, which is also what the walk in the opposite sense gives.  The definition
# is what the header states and what every other check here relies on; both lists are asserted, one through the other.
ISSUE_DISC_EDGES = {2: 0, 5: 0, 12: 2, 60: 7, 100: 0}


@pytest.fixture(scope="module")
def results():
    """name -> (brute, restatement) of every named and fuzz case, computed once"""
    return {name: (cases.run_brute(c), cases.run_ref(c)) for name, c in {**NAMED, **FUZZ}.items()}


def test_header_declares_the_stage():
    txt = open(os.path.join(ROOT, "include", "bs_api.h")).read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    assert "#define BS_API_VERSION 5" in txt and L.bs_api_version() == 5
    assert f"#define BS_HULL_MAX_SIDE {_lib.HULL_MAX_SIDE}" in txt and f"#define BS_HULL_ROUND_BATCH {_lib.HULL_ROUND_BATCH}" in txt
    assert (brute.MAX_SIDE, ref.ROUND_BATCH) == (_lib.HULL_MAX_SIDE, _lib.HULL_ROUND_BATCH)
    for name in ("label_hulls", "label_hulls_dev", "label_hulls_emit_dev", "building_boxes", "write_boxes_obj", "LabelHulls"):
        assert callable(getattr(hulls, name))


def test_brute_against_qhull(results):
    from scipy.spatial import ConvexHull
    for name, (lab, nl) in {**NAMED, **FUZZ}.items():
        b = results[name][0]
        for l in np.nonzero(b.status == brute.OK)[0]:
            pts = np.array(sorted(brute.corners(lab, l)))
            q = ConvexHull(pts)
            assert abs(2 * q.volume - int(b.hull_area2[l])) <= 1e-9 * max(1, int(b.hull_area2[l])), (name, l)
            mine = {tuple(p) for p in b.hull_xy[b.hull_offset[l]:b.hull_offset[l + 1]].tolist()}
            assert mine <= {tuple(p) for p in pts[q.vertices].tolist()}, (name, l)


def test_box_against_every_pair_direction(results):
    """the least rectangle over the directions p - q of every pair of hull vertices, as fractions, is the box"""
    for name, (b, _) in results.items():
        for l in np.nonzero(b.status == brute.OK)[0]:
            ring = [tuple(int(v) for v in p) for p in b.hull_xy[b.hull_offset[l]:b.hull_offset[l + 1]]]
            if len(ring) > 24:
                continue
            least = None
            for p in ring:
                for q in ring:
                    d = (p[0] - q[0], p[1] - q[1])
                    if d == (0, 0):
                        continue
                    a = [v[0] * d[0] + v[1] * d[1] for v in ring]
                    c = [v[1] * d[0] - v[0] * d[1] for v in ring]
                    area = Fraction((max(a) - min(a)) * (max(c) - min(c)), d[0] * d[0] + d[1] * d[1])
                    least = area if least is None or area < least else least
            assert least == Fraction(int(b.area_num[l]), int(b.len2[l])), (name, l)


def test_identities_and_restatement(results):
    for name, (b, r) in results.items():
        brute.identities(b)
        assert brute.same(b, r) is None, (name, brute.same(b, r))
        assert r.info["n_candidates"] >= b.n_hull_vertices and r.info["max_live"] <= r.info["n_candidates"], name


def test_smallest_shapes(results):
    one = results["one_pixel"][0]
    assert one.n_hull.tolist() == [4] and one.hull_xy.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]] and one.area_num[0] == one.len2[0]
    rect = results["full_rectangle"][0]
    assert (rect.n_hull[0], rect.best_edge[0], rect.area_num[0]) == (4, 0, 9 * 5 * rect.len2[0])
    sq = results["square"][0]
    assert (sq.n_hull[0], sq.best_edge[0], sq.area_num[0]) == (4, 0, 36 * sq.len2[0]) and sq.box[0].tolist() == [2, 2, 8, 8]
    assert results["diamond"][0].n_hull[0] == 8 and results["corner_touch"][0].n_hull[0] == 6
    ring = results["ring_shaped"][0]
    assert ring.n_hull[0] == 4 and ring.hull_area2[0] > ring.pixels2[0]  # (the hole adds nothing to the hull)
    assert results["three_far_pieces"][0].box[0].tolist() == [2, 1, 48, 38]
    un = results["unused_labels"][0]
    assert un.status.tolist() == [1, 0, 1, 1, 0, 1, 1] and (un.n_ok, un.n_empty) == (2, 5)
    no = results["nothing"][0]
    assert no.n_empty == 3 and no.n_hull_vertices == 0 and no.hull_xy.shape == (0, 2)
    assert results["touches_all_borders"][0].box[0].tolist() == [0, 0, 11, 9]
    for w, h in cases.LINE_SIZES:
        b = results[f"full_line_{w}x{h}"][0]
        assert (b.n_hull[0], b.best_edge[0], b.area_num[0]) == (4, 0, w * h * b.len2[0])


def test_hull_sizes(results):
    for r, (n_hull, edge) in cases.DISCS.items():
        b = results[f"disc_{r}"][0]
        assert (b.n_hull[0], b.best_edge[0]) == (n_hull, edge)
        assert (b.best_edge[0] - 1) % n_hull == ISSUE_DISC_EDGES[r]
    for j in cases.PARABOLAS:
        assert results[f"parabola_{j}"][0].n_hull[0] == j + 5
    assert {results[f"parabola_{j}"][0].n_hull[0] for j in (58, 59, 60)} == {63, 64, 65}  # around the 64 lanes of the box pass


def test_rotated_rectangles(results):
    for d, a, b_, n in cases.ROTATED:
        b = results[f"rotated_{d[0]}_{d[1]}_{a}x{b_}"][0]
        dx, dy = (int(v) for v in b.dir[0])
        assert dx * d[1] - dy * d[0] == 0 or dx * d[0] + dy * d[1] == 0, (d, dx, dy)


def test_moving_a_label_changes_only_its_place():
    for name in ("L", "diamond", "disc_12", "rotated_7_3_33x20", "corner_touch"):
        a, b = cases.run_brute(NAMED[name]), cases.run_brute(cases.moved(NAMED[name], 5, 3))
        for k in brute.PER_LABEL + brute.TOTALS:
            if k != "box":
                assert np.array_equal(getattr(a, k), getattr(b, k)), (name, k)
        assert np.array_equal(a.box + [5, 3, 5, 3], b.box) and np.array_equal(a.hull_xy + [5, 3], b.hull_xy)


def test_large_cases_of_the_restatement():
    """the serpentine (one ring of more than 2^16 half-edges, a hull of 4), the bound, the 1025 x 1027 blobs"""
    c = cases.serpentine()
    b, r = cases.run_brute(c), cases.run_ref(c)
    assert brute.same(b, r) is None and b.n_hull.tolist() == [4] and r.info["n_candidates"] > 256
    c = cases.bound()
    b, r = cases.run_brute(c), cases.run_ref(c)
    assert brute.same(b, r) is None and b.status.tolist() == [brute.TOO_LARGE, brute.OK] and b.n_hull.tolist() == [0, 4]
    assert b.box.tolist() == [[0, 0, 16385, 1], [0, 1, 16383, 2]] and b.pixels2.tolist() == [2 * 16385, 2 * 16383]
    assert b.area_num[0] == 0 and b.len2[0] == 0
    c = cases.blobs()
    b, r = cases.run_brute(c), cases.run_ref(c)
    assert brute.same(b, r) is None and b.n_ok > 1000
    brute.identities(b)


# ---- the host-only functions of the library ------------------------------------------------------------------------------
def test_corner_rounding():
    assert [brute.round_div(n, 2) for n in (-3, -2, -1, 0, 1, 2, 3)] == [-2, -1, -1, 0, 1, 1, 2]
    L = _lib.load()
    for name in ("one_pixel", "L", "diamond", "disc_5", "rotated_4_3_41x17", "rotated_7_3_33x20", "parabola_10", "three_far_pieces"):
        b = cases.run_brute(NAMED[name])
        st, keep = hulls._label_hulls_struct(b)
        for bin_, origin in ((1, None), (7, [3, -2]), (100, [-123456, -98765]), (333, [-10 ** 9, 5])):
            org = None if origin is None else np.array(origin, np.int32)
            for l in range(b.n_labels):
                out = np.zeros((4, 2), np.int64)
                rc = L.bs_hull_box_corners(C.byref(st), l, bin_, api._ptr(org), out.ctypes.data)
                if b.status[l] != brute.OK:
                    assert rc == -1
                    continue
                assert rc == 0 and out.tolist() == brute.box_corners(b, l, bin_, origin), (name, l, bin_)
        assert L.bs_hull_box_corners(C.byref(st), b.n_labels, 1, None, np.zeros((4, 2), np.int64).ctypes.data) == -1
        assert L.bs_hull_box_corners(C.byref(st), 0, 0, None, np.zeros((4, 2), np.int64).ctypes.data) == -1
    # the conveniences of the binding come from the same integers
    b = cases.run_brute(NAMED["rotated_4_3_100x50"])
    h = hulls.LabelHulls(b.width, b.image_height, b.n_labels, b.n_hull_vertices, b.n_ok, b.n_empty, b.n_too_large,
                       **{k: getattr(b, k) for k in brute.PER_LABEL}, hull_xy=b.hull_xy)
    assert h.corners(0, 7, [3, -2, 9]).tolist() == brute.box_corners(b, 0, 7, [3, -2])
    assert abs(h.angle_deg[0] - np.degrees(np.arctan2(3, 4))) < 1e-9 and 0 <= h.angle_deg[0] < 90
    assert 95 < h.long_side[0] < 105 and 45 < h.short_side[0] < 55 and 0.9 < h.rectangularity[0] <= h.convexity[0] <= 1


def test_writer_bytes(tmp_path):
    for name, bin_, origin in (("unused_labels", 100, None), ("three_far_pieces", 25, [-5000, -70000, -300]),
                               ("rotated_5_2_80x33", 7, [11, -13, 17]), ("nothing", 10, None)):
        b = cases.run_brute(NAMED[name])
        path = tmp_path / f"{name}.obj"
        hulls.write_boxes_obj(b, path, bin_, origin)
        assert path.read_bytes() == brute.obj_text(b, bin_, origin).encode(), name
    b = cases.run_brute(NAMED["L"])
    b.hull_offset = b.hull_offset[:1]
    with pytest.raises(ValueError):
        hulls.write_boxes_obj(b, tmp_path / "bad.obj", 100)
    b = cases.run_brute(NAMED["L"])
    with pytest.raises(api.BsError):
        hulls.write_boxes_obj(b, tmp_path / "bad.obj", 0)
    z = _lib.LabelHulls()
    _lib.load().bs_label_hulls_free(C.byref(z))  # a zeroed struct


# ---- sparse cases: the compared products around 2^64, the coordinates at the bound, the batches of rounds -------------------
# The device compares area_num_i * len2_j with area_num_j * len2_i by high word, then low word (less_product of bs_hull.hip);
# the host build of the same function is one 128-bit comparison, so nothing here can stand in for the device.  What can be
# asserted here is that the cases ask what they were built to ask: the class of every pair of products the least rectangle
# depends on (the pairs with the best edge or an edge tied with it), and the edge a comparison of the low words alone gives.
MAGNITUDE = cases.magnitude_cases()
ROUNDS = cases.round_cases()
SPARSE_FUZZ = {f"sparse_fuzz_{s}": cases.sparse_fuzz(s) for s in range(cases.N_SPARSE_FUZZ)}
SPARSE = {**MAGNITUDE, **ROUNDS, **SPARSE_FUZZ}
T64 = 1 << 64


@functools.lru_cache(maxsize=None)
def sparse_pair(name):
    """(definition, restatement) of a sparse case from its pixel list, computed once"""
    s = cases.full_bound() if name == "full_bound" else SPARSE[name]
    return cases.sparse_brute(s), cases.sparse_ref(s)


def product_class(p1, p2):
    """(a) both below 2^64, (b) the high words differ, (c) they are equal and not zero and the low words decide, (d) equal
    products at or above 2^64"""
    if p1 < T64 and p2 < T64:
        return "a"
    if p1 == p2:
        return "d"
    return "b" if p1 >> 64 != p2 >> 64 else "c"


def compared(b, l=0):
    """(products, tied, pairs) of label l: (area_num, len2) of every hull edge, the edges tied at the least area, and for
    every ordered pair (i, j) with i or j among them the two products area_num_i * len2_j, area_num_j * len2_i"""
    pr = brute.edge_products(brute.ring_of(b, l))
    e = int(b.best_edge[l])
    assert pr[e] == (int(b.area_num[l]), int(b.len2[l]))
    tied = [i for i in range(len(pr)) if pr[i][0] * pr[e][1] == pr[e][0] * pr[i][1]]
    assert tied[0] == e and all(pr[e][0] * pr[i][1] <= pr[i][0] * pr[e][1] for i in range(len(pr)))
    pairs = {(i, j): (pr[i][0] * pr[j][1], pr[j][0] * pr[i][1]) for i in range(len(pr)) for j in range(len(pr))
             if i != j and (i in tied or j in tied)}
    return pr, tied, pairs


def classes(pairs):
    return {product_class(*p) for p in pairs.values()}


def low_less(pr, i, j):
    """edge i before edge j by the low words of the two products alone"""
    return (pr[i][0] * pr[j][1]) % T64 < (pr[j][0] * pr[i][1]) % T64


def test_sparse_definition_against_restatement_qhull_and_pair_directions():
    from scipy.spatial import ConvexHull
    for name in list(SPARSE) + ["full_bound"]:
        b, r = sparse_pair(name)
        brute.identities(b)
        assert brute.same(b, r) is None, (name, brute.same(b, r))
        s = cases.full_bound() if name == "full_bound" else SPARSE[name]
        for l in np.nonzero(b.status == brute.OK)[0]:
            ring = brute.ring_of(b, l)
            p = s["pixels"][s["pixels"][:, 2] == l]
            pts = np.unique(np.concatenate([p[:, :2] + d for d in ((0, 0), (1, 0), (0, 1), (1, 1))]), axis=0)
            q = ConvexHull(pts)
            assert abs(2 * q.volume - int(b.hull_area2[l])) <= 1e-9 * int(b.hull_area2[l]), (name, l)
            assert set(ring) <= {tuple(v) for v in pts[q.vertices].tolist()}, (name, l)
            if len(ring) > 24:
                continue
            least = None
            for u in ring:
                for v in ring:
                    d = (u[0] - v[0], u[1] - v[1])
                    if d != (0, 0):
                        a, c = [w[0] * d[0] + w[1] * d[1] for w in ring], [w[1] * d[0] - w[0] * d[1] for w in ring]
                        area = Fraction((max(a) - min(a)) * (max(c) - min(c)), d[0] * d[0] + d[1] * d[1])
                        least = area if least is None or area < least else least
            assert least == Fraction(int(b.area_num[l]), int(b.len2[l])), (name, l)
    # the image and its pixel list are one case to both references
    for name in ("ladder_1024", "rounds_1_5_9", "tie_diamond_beside"):
        b, r = sparse_pair(name)
        c = cases.dense(SPARSE[name])
        assert brute.same(cases.run_brute(c), b) is None and brute.same(cases.run_ref(c), r, ("n_candidates", "rounds", "max_live")) is None


def test_products_on_both_sides_of_two_to_the_64():
    # the ladder: one shape, its side growing through the crossing
    got = {}
    for side in cases.LADDER_SIDES:
        b = sparse_pair(f"ladder_{side}")[0]
        pr, tied, pairs = compared(b)
        assert (b.n_hull[0], tied) == (8, [3]) and b.dir[0].all() and b.box[0].tolist() == [0, 0, side, side]
        got[side] = classes(pairs)
    assert got[1024] == got[1200] == got[1500] == {"a"} and got[4096] == {"b"}, got
    assert got[2048] == {"a", "c"}, got  # (the crossing itself: some pairs on either side)
    assert max(max(p) for p in compared(sparse_pair("ladder_1500")[0])[2].values()) < T64 // 4  # 1500: still two bits below
    assert min(min(p) for p in compared(sparse_pair("ladder_4096")[0])[2].values()) >= 4 * T64
    # the high word decides against the low word: by the low words alone edge 5 comes before every other edge, whichever
    # order they are compared in, and the least rectangle stands on edge 3
    for name in ("high_word", "high_word_beside"):
        b = sparse_pair(name)[0]
        pr, tied, pairs = compared(b)
        assert (b.n_hull[0], tied) == (8, [3])
        assert all(low_less(pr, 5, j) for j in range(8) if j != 5)
        p3, p5 = pairs[3, 5]
        assert p3 < p5 and p3 >> 64 < p5 >> 64 and p3 % T64 > p5 % T64
        scan = 0
        for i in range(1, 8):  # the definition's own scan, by the low words
            scan = i if low_less(pr, i, scan) else scan
        assert scan == 5 != b.best_edge[0]
        assert {"b", "c"} <= classes(pairs)
    # high words equal and not zero: mirror images but for one pixel, the two least rectangles 2^-12.9 apart
    b = sparse_pair("class_c")[0]
    pr, tied, pairs = compared(b)
    runner = sorted(range(len(pr)), key=lambda i: Fraction(*pr[i]))[1]
    assert (tied, runner) == ([3], 5) and product_class(*pairs[3, 5]) == "c" and min(pairs[3, 5]) >= T64
    # the tie above 2^64: the four long edges of the diamond, the lowest wins; they beat the axis-parallel rectangle
    for name, l in (("tie_diamond", 0), ("tie_diamond_beside", 1)):
        b = sparse_pair(name)[0]
        pr, tied, pairs = compared(b, l)
        assert (b.n_hull[l], tied, b.best_edge[l]) == (8, [1, 3, 5, 7], 1) and b.len2[l] == 2 * 1500 ** 2
        assert all(product_class(*pairs[i, j]) == "d" for i in tied for j in tied if i != j) and pr[1][0] * pr[1][1] >= 4 * T64
        assert all(pr[i][1] == 1 and Fraction(*pr[i]) == 3001 ** 2 > Fraction(*pr[1]) for i in (0, 2, 4, 6))
    # the same tie with more than 64 hull vertices: the tied edges in four lanes of a wave-wide reduction, one of them beyond
    # 64; and with 128, where edges 64 apart tie
    b = sparse_pair("tie_diamond_lanes")[0]
    pr, tied, pairs = compared(b)
    assert (b.n_hull[0], tied) == (96, [12, 36, 60, 84]) and len({i % 64 for i in tied}) == 4
    assert all(product_class(*pairs[i, j]) == "d" for i in tied for j in tied if i != j)
    b = sparse_pair("tie_diamond_same_lane")[0]
    pr, tied, pairs = compared(b)
    assert (b.n_hull[0], tied) == (128, [16, 48, 80, 112]) and product_class(*pairs[16, 80]) == product_class(*pairs[48, 112]) == "d"
    # the second label of an image: small, and whole
    for name, l in (("high_word_beside", 1), ("tie_diamond_beside", 0)):
        b = sparse_pair(name)[0]
        assert b.status.tolist() == [brute.OK, brute.OK] and (b.n_hull[l], b.pixels2[l], b.hull_area2[l]) == (5, 6, 7)


def test_coordinates_at_the_bound():
    b = sparse_pair("bound_transposed")[0]
    assert b.status.tolist() == [brute.TOO_LARGE, brute.OK] and b.box.tolist() == [[0, 0, 1, 16385], [1, 0, 2, 16383]]
    assert b.hull_xy.tolist() == [[1, 0], [2, 0], [2, 16383], [1, 16383]]
    for name, k in (("strip", 0), ("strip_transposed", 1)):
        b = sparse_pair(name)[0]
        box = [0, 0, 16383, 2048] if k == 0 else [0, 0, 2048, 16383]
        assert b.status.tolist() == [brute.TOO_LARGE, brute.OK] and b.box[1].tolist() == box and b.n_hull[1] == 9
        ring = brute.ring_of(b, 1)
        assert (0, 0) in ring and tuple(box[2:]) in ring and b.dir[1].all()
        pr, tied, pairs = compared(b, 1)
        assert max(p[1] for p in pr) > 2 ** 26 and classes(pairs) == {"a", "b"}  # (edges beyond 8 192 long)
    # both axes: the box is the bound in both, the rectangle oblique, the products with the best edge above 2^84
    b = sparse_pair("full_bound")[0]
    pr, tied, pairs = compared(b)
    assert b.box[0].tolist() == [0, 0, 16383, 16383] and b.n_hull[0] == 8 and tied == [1] and b.dir[0].all()
    top = sorted(max(pairs[1, j]) for j in range(8) if j != 1)
    assert top[-2] > 2 ** 84 and 2 ** 84.8 < top[-1] < 2 ** 87


def test_round_counts_around_the_batch():
    assert ref.ROUND_BATCH == 4
    for n in cases.ROUND_CHAINS:
        assert sparse_pair(f"rounds_{n}")[1].info["rounds"] == n
    assert sorted(cases.ROUND_CHAINS) == [5, 8, 9, 13]  # 5: three idle rounds; 8: ends on a read; 9, 13: a third, a fourth batch
    s = SPARSE["rounds_1_5_9"]
    alone = [cases.sparse_ref(cases.one_label(s["width"], s["height"], s["pixels"][s["pixels"][:, 2] == l][:, :2])) for l in range(3)]
    assert [a.info["rounds"] for a in alone] == [1, 5, 9] and sparse_pair("rounds_1_5_9")[1].info["rounds"] == 9


def test_corners_and_writer_at_these_magnitudes(tmp_path):
    """bs_hull_box_corners and the OBJ writer against fractions: num * bin needs more than 64 bits from the ladder on"""
    L = _lib.load()

    def rounded(f):  # half away from zero
        q = (abs(f) + Fraction(1, 2)).__floor__()
        return -q if f < 0 else q

    most = 0
    for name in list(MAGNITUDE) + ["full_bound"]:
        b = sparse_pair(name)[0]
        st, keep = hulls._label_hulls_struct(b)
        for bin_, origin in ((1, None), (1000, [-123456, 98765, 7]), (2 ** 31 - 1, [2 ** 31 - 1, -2 ** 31, 0])):
            org = None if origin is None else np.array(origin, np.int32)
            for l in np.nonzero(b.status == brute.OK)[0]:
                s = brute.ring_of(b, l)[int(b.best_edge[l])]
                d, len2 = [int(v) for v in b.dir[l]], int(b.len2[l])
                a0, a1, c = (Fraction(int(v), len2) for v in (b.a_min[l], b.a_max[l], b.c_max[l]))
                want = [[s[0] + a * d[0] - n * d[1], s[1] + a * d[1] + n * d[0]] for a, n in ((a0, 0), (a1, 0), (a1, c), (a0, c))]
                want = [[rounded(x * bin_) + (origin or [0, 0])[0], rounded(y * bin_) + (origin or [0, 0])[1]] for x, y in want]
                assert brute.box_corners(b, l, bin_, origin) == want, (name, l, bin_)
                out = np.zeros((4, 2), np.int64)
                assert L.bs_hull_box_corners(C.byref(st), int(l), bin_, api._ptr(org), out.ctypes.data) == 0
                assert out.tolist() == want, (name, l, bin_)
                most = max(most, int(b.c_max[l]) * max(abs(d[0]), abs(d[1])) * bin_)
            path = tmp_path / f"{name}_{bin_}.obj"
            hulls.write_boxes_obj(b, path, bin_, origin)
            assert path.read_bytes() == brute.obj_text(b, bin_, origin).encode(), (name, bin_)
    assert most > 2 ** 72  # (c_max * dy * bin of the full bound: far beyond 64 bits)


def test_corner_index_needs_its_14_bits(monkeypatch):
    """`shallow` is the case for the width of the corner index: two hull vertices more than 8 192 apart in x whose rows differ
    by one.  The restatement with a shift of 13 starts its list elsewhere there and nowhere else, the full bound included."""
    want = {name: name == "shallow" for name in ("shallow", "shallow_transposed", "strip", "strip_transposed", "bound_transposed",
                                                 "full_bound")}
    monkeypatch.setattr(ref, "CORNER_SHIFT", 13)
    for name, differs in want.items():
        s = cases.full_bound() if name == "full_bound" else SPARSE[name]
        assert (brute.same(sparse_pair(name)[0], cases.sparse_ref(s)) is not None) == differs, name
    b = sparse_pair("shallow")[0]
    assert b.box[0].tolist() == [0, 0, 16383, 4] and b.hull_xy[0].tolist() == [16382, 0] and [0, 1] in b.hull_xy.tolist()
