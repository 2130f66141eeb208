"""Roof evidence in numpy (include/bs_api.h, "roof evidence"): the counts by bincount, the window sums from an integral image,
checked against tests/evidence_ref/brute.py; the quality rule of the planes; and the footprints under the screen restated on
tests/footprint_ref."""
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


brute = _load("evidence_brute", os.path.join(HERE, "brute.py"))
gref = _load("ground_ref", os.path.join(TESTS, "ground_ref", "ground_ref.py"))
FIGURES, IMAGES, params = brute.FIGURES, brute.IMAGES, brute.params


def window_sums(a, r):
    """int64 [h][w]: the sum of a over the square of radius r around every pixel, clipped to the image"""
    h, w = a.shape
    ii = np.zeros((h + 1, w + 1), np.int64)
    ii[1:, 1:] = np.cumsum(np.cumsum(a.astype(np.int64), 0), 1)
    y0, y1 = np.maximum(np.arange(h) - r, 0), np.minimum(np.arange(h) + r + 1, h)
    x0, x1 = np.maximum(np.arange(w) - r, 0), np.minimum(np.arange(w) + r + 1, w)
    return ii[y1][:, x1] - ii[y0][:, x1] - ii[y1][:, x0] + ii[y0][:, x0]


def evidence(xyz, plane_idx, n_planes, plane_ok, extent, bin, ground_th, p, model=None):
    """SimpleNamespace: width, height, keep (uint8 [h][w]), above, planar, win_above, win_planar (int32 [h][w]) and every
    name of FIGURES.  model = (dtm, cell, min_height) or None.  Raises the errors of brute.check."""
    w, h = brute.check(xyz, plane_idx, n_planes, plane_ok, extent, bin, p)
    q = np.asarray(xyz, dtype=np.int64)
    px, py = q[:, 0] // bin, q[:, 1] // bin
    if (q[:, :2] < 0).any() or (px >= w).any() or (py >= h).any():
        raise brute.RangeError("xy")
    counts = ~gref.below(q, ground_th, model)
    lab = np.asarray(plane_idx, dtype=np.int64)
    good = (lab >= 1) & (lab <= n_planes)
    if plane_ok is not None and n_planes:
        ok = np.asarray(plane_ok) != 0
        good &= ok[np.clip(lab - 1, 0, n_planes - 1)]
    pix = py * w + px
    above = np.bincount(pix[counts], minlength=w * h).reshape(h, w)
    planar = np.bincount(pix[counts & good], minlength=w * h).reshape(h, w)
    A, P = window_sums(above, p["r"]), window_sums(planar, p["r"])
    enough, share = A >= p["min_points"], P * p["den"] >= p["num"] * A
    out = SimpleNamespace(width=w, height=h, keep=(enough & share).astype(np.uint8), above=above.astype(np.int32),
                          planar=planar.astype(np.int32), win_above=A.astype(np.int32), win_planar=P.astype(np.int32))
    out.n_counted, out.n_planar = int(above.sum()), int(planar.sum())
    out.n_pixels = int((above > 0).sum())
    out.pixels_kept = int((enough & share).sum())
    out.pixels_rejected = int((enough & ~share).sum())
    out.pixels_thin = int(((A > 0) & ~enough).sum())
    out.max_window = int(A.max())
    return out


def same(a, b):
    """None if the restatement's result a equals the brute force's dict b everywhere, else the name that differs"""
    for k in ("width", "height") + FIGURES:
        if getattr(a, k) != b[k]:
            return k
    for k in IMAGES:
        if not np.array_equal(np.asarray(getattr(a, k), np.int64), np.asarray(b[k], np.int64)):
            return k
    return None


def plane_fit_figures(xyz, plane_idx, n_planes):
    """(status, n_points, r_sq_sum) per plane of tests/fit_ref, the restatement the device's bs_plane_fit equals"""
    fit = _load("fit_ref", os.path.join(TESTS, "fit_ref", "fit_ref.py")).plane_fit(xyz, plane_idx, n_planes)
    return fit.status, fit.n_points, fit.r_sq_sum


def plane_quality(status, n_points, r_sq_sum, min_points=0, max_rms=100):
    return np.array(brute.plane_quality(status, n_points, r_sq_sum, min_points, max_rms), np.uint8).reshape(-1)


def rms(n_points, r_sq_sum):
    """f64 [n_planes]: the rms residual in millimetres, inf without a point"""
    n = np.asarray(n_points, np.float64)
    return np.where(n > 0, np.sqrt(np.asarray(r_sq_sum, np.float64) / np.maximum(n, 1)), np.inf)


# ---- the footprints under the screen --------------------------------------------------------------------------------------
def _fref():
    sys.path.insert(0, os.path.join(TESTS, "footprint_ref"))
    import ref as fref
    return fref


def screened_mask(image, keep, threshold=10):
    """uint8 [h][w] 0 / 1: foreground iff q > threshold and keep != 0"""
    return (_fref().mask(image, threshold) != 0).astype(np.uint8) & (np.asarray(keep) != 0)


def screened_footprints(image, keep, threshold=10, kernel_size=5, iterations=2):
    """(Result of tests/footprint_ref, closed mask 0 / 1) of bs_footprints while `keep` is the screen"""
    fref = _fref()
    closed = fref.close(screened_mask(image, keep, threshold), kernel_size, iterations) if iterations else \
        screened_mask(image, keep, threshold)
    return fref.find_contours(closed), (closed != 0).astype(np.uint8)


def building_chain(xyz, ground_th, model=None, keep=None, bin=100):
    """(mask before the closing, building map object of tests/building_ref) of the reference chain: the pixels that a counting
    point touches, AND keep where it is given, closed, labelled"""
    sys.path.insert(0, os.path.join(TESTS, "building_ref"))
    import building_ref as bref
    fref = _fref()
    m = gref.splat_mask(xyz, ~gref.below(xyz, ground_th, model), np.asarray(xyz).max(0), bin)
    if keep is not None:
        m = m & (np.asarray(keep) != 0)
    _, closed = fref.footprints(fref.image_of_mask(m))
    return m, bref.building_map(closed)
