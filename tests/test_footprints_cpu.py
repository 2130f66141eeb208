"""Footprint contours (extracted_contour, my_function.cpp:8-145) without a GPU: the sequential restatement in
tests/footprint_ref/contour_ref.c against hand-written expectations, scipy's morphology and the reference's own
density PNGs, the OBJ format, and the C-ABI surface of bs_footprints."""
import glob
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
import ref  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "raster_*.npz")))


def _pts(r):
    return [c.tolist() for c in r.contours]


def _mask(shape, *boxes):
    m = np.zeros(shape, np.uint8)
    for y0, y1, x0, x1 in boxes:
        m[y0:y1, x0:x1] = 1
    return m


def test_ellipse_5x5_is_the_literal():
    lit = ["00100", "11111", "11111", "11111", "00100"]
    assert ref.ellipse(5).tolist() == [[int(c) for c in row] for row in lit]
    assert ref.ellipse(1).tolist() == [[1]]
    assert ref.ellipse(3).tolist() == [[0, 1, 0], [1, 1, 1], [0, 1, 0]]  # dx(+-1) = round(0)
    assert ref.ellipse(7)[0].tolist() == [0, 0, 0, 1, 0, 0, 0]


def test_rectangle():
    r = ref.find_contours(_mask((8, 9), (2, 6, 3, 7)))
    assert _pts(r) == [[[3, 2], [3, 5], [6, 5], [6, 2]]]
    assert r.area.tolist() == [9.0] and r.perimeter.tolist() == [12.0]


def test_single_pixel():
    r = ref.find_contours(_mask((5, 5), (2, 3, 3, 4)))
    assert _pts(r) == [[[3, 2]]] and r.area.tolist() == [0.0] and r.perimeter.tolist() == [0.0]


def test_horizontal_and_vertical_runs():
    assert _pts(ref.find_contours(_mask((5, 9), (2, 3, 1, 7)))) == [[[1, 2], [6, 2]]]
    assert _pts(ref.find_contours(_mask((9, 5), (1, 7, 2, 3)))) == [[[2, 1], [2, 6]]]


def test_diagonal_line():
    m = np.zeros((6, 6), np.uint8)
    for k in range(1, 5):
        m[k, k] = 1
    assert _pts(ref.find_contours(m)) == [[[1, 1], [4, 4]]]


def test_l_shape():
    m = _mask((8, 8), (1, 6, 1, 3), (4, 6, 1, 6))
    # the inner corner is cut diagonally: (2, 4) is skipped by the 8-connected follower
    assert _pts(ref.find_contours(m)) == [[[1, 1], [1, 5], [5, 5], [5, 4], [3, 4], [2, 3], [2, 1]]]


def test_ring_gives_only_the_outer_contour_and_drops_a_blob_in_its_hole():
    ring = _mask((12, 12), (1, 11, 1, 11))
    ring[3:9, 3:9] = 0
    assert _pts(ref.find_contours(ring)) == [[[1, 1], [1, 10], [10, 10], [10, 1]]]
    ring[5:7, 5:7] = 1  # a blob inside the hole: not external
    assert _pts(ref.find_contours(ring)) == [[[1, 1], [1, 10], [10, 10], [10, 1]]]


def test_two_blobs_bottom_one_first():
    r = ref.find_contours(_mask((12, 10), (1, 3, 1, 4), (7, 9, 5, 8)))
    assert _pts(r) == [[[5, 7], [5, 8], [7, 8], [7, 7]], [[1, 1], [1, 2], [3, 2], [3, 1]]]


def test_edge_touching_blob_is_traced():
    r = ref.find_contours(_mask((4, 5), (0, 4, 0, 5)))
    assert _pts(r) == [[[0, 0], [0, 3], [4, 3], [4, 0]]]


def test_checkerboard_is_one_8_connected_component():
    m = (np.indices((6, 6)).sum(0) % 2 == 0).astype(np.uint8)
    r = ref.find_contours(m)
    assert len(r.contours) == 1 and r.contours[0][0].tolist() == [0, 0]


def _scipy_close(m, s, k):
    import scipy.ndimage as nd
    st = ref.ellipse(s).astype(bool)
    d = nd.binary_dilation(m.astype(bool), st, iterations=k, border_value=0) if k else m.astype(bool)
    return nd.binary_erosion(d, st, iterations=k, border_value=1) if k else d


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (41, 1), (17, 23), (64, 65), (90, 33)])
@pytest.mark.parametrize("s,k", [(5, 2), (5, 1), (3, 3), (7, 2), (1, 2), (5, 0)])
def test_close_matches_scipy(shape, s, k):
    rng = np.random.default_rng(hash((shape, s, k)) % 2**32)
    m = (rng.random(shape) < 0.35).astype(np.uint8)
    assert np.array_equal(ref.close(m, s, k).astype(bool), _scipy_close(m, s, k))


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_mask_matches_reference_density_png(path):
    """The restatement's quantised threshold equals the reference's own PNG channel read back and thresholded."""
    g = np.load(path)
    assert np.array_equal(ref.mask(g["image"]), (g["png_density"][..., 1] > 10).astype(np.uint8))
    # and it is exactly "density sum != 0": the +-1 quantisation slack of the PNG cannot cross the threshold
    assert np.array_equal(ref.mask(g["image"]).astype(bool), g["image"][..., 1] != 0)


def test_obj_lines_are_float32_g(tmp_path):
    m = _mask((7, 9), (1, 4, 2, 7), (5, 6, 0, 1))
    r = ref.find_contours(m)
    p = tmp_path / "a.obj"
    r.write_obj(p)
    lines = p.read_text().split("\n")
    assert lines[1] == f"# contours: {len(r.contours)}" and lines[3] == ""
    exp_v, exp_f, base = [], [], 1
    for c in r.contours:
        for x, y in c:
            fx = np.float32(np.float32(x) / np.float32(9))
            fy = np.float32(np.float32(1.0) - np.float32(y) / np.float32(7))
            exp_v += ["v %g %g 0.0" % (float(fx), float(fy)), "v %g %g 1" % (float(fx), float(fy))]
        n = len(c)
        exp_f += [f"f {base + 2 * i} {base + 2 * ((i + 1) % n)} {base + 2 * ((i + 1) % n) + 1} {base + 2 * i + 1}"
                  for i in range(n)]
        base += 2 * n
    assert [ln for ln in lines if ln.startswith("v ")] == exp_v
    assert [ln for ln in lines if ln.startswith("f ")] == exp_f


def test_library_obj_writer_matches_restatement(tmp_path):
    """api.write_footprints_obj goes through bs_contours_write_obj (host code, no GPU needed)."""
    from buildingsegment_amd import api, build
    build.build()
    rng = np.random.default_rng(5)
    m = _scipy_close((rng.random((40, 57)) < 0.2).astype(np.uint8), 5, 1).astype(np.uint8)
    r = ref.find_contours(m)
    fp = api.Footprints(r.contours, r.area, r.perimeter, 57, 40)
    api.write_footprints_obj(fp, tmp_path / "lib.obj")
    r.write_obj(tmp_path / "ref.obj")
    assert (tmp_path / "lib.obj").read_bytes() == (tmp_path / "ref.obj").read_bytes()


def test_footprint_exports_are_declared_and_loaded():
    from buildingsegment_amd import _lib, build
    txt = open(os.path.join(os.path.dirname(HERE), "include", "bs_api.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(bs_[a-z_]+)\s*\(", txt))
    new = {"bs_footprints_dev", "bs_footprints", "bs_contours_free", "bs_contours_write_obj"}
    assert new <= declared and new <= set(_lib.EXPORTS)
    build.build()
    L = _lib.load()
    for s in new:
        assert hasattr(L, s), s
    c = _lib.Contours()
    L.bs_contours_free(c)  # a zeroed struct is fine
    assert L.bs_footprints(None, None, 1, 1, 10, 5, 2, None, None, None) == -1
