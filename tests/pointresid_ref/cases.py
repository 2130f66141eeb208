"""Cases for the point residuals (include/bs_api.h, "point residuals"): the runs of tests/modelraster_ref/cases.py by import
and the stage's own shapes, each with a pixel edge and seeded point sets, and `regimes`: which rows of the threshold table
("Point residuals") a run reaches, worked out from the restatement's result and trace."""
from __future__ import annotations

import importlib.util
import math
import os
import sys
import zlib
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


mc = _load("modelraster_cases", os.path.join(HERE, "..", "modelraster_ref", "cases.py"))
pref = _load("pointresid_ref", os.path.join(HERE, "pointresid_ref.py"))
brute, mref, tc, sc, tbrute = pref.brute, mc.mref, mc.tc, mc.sc, mc.tbrute

REGIMES = ("tie_owned", "tie_not_owned", "multi", "uncovered", "failed_label", "long_list", "empty_pixel", "span_over_chunk",
           "labels_below_cap", "labels_at_cap", "labels_above_cap", "height_wide", "height_narrow", "above", "below", "plane_agrees",
           "plane_differs")
STRIPS = (pref.FIG_CAP - 1, pref.FIG_CAP, pref.FIG_CAP + 1, 5000)
BINS = (1, 3, 4, 25, 100)  # the pixel edge of an imported run, by its name
Z_MAX = (1 << 24) - 1
CLIP2 = 60       # the inlier bound of every run's cloud: the noise stays inside it, the far share does not
PAIRS = 60_000   # random points of a run: about this many (point, triangle) pairs
TIE_CAP = 400    # tie points of a run
N_PLANES = 4


def slope(z):
    """one facet of 200 x 200 pixels whose tops run from -z at the left edge to +z at the right one"""
    n = 200
    X = np.arange(n)[None, :, None] + (np.arange(4) & 1)[None, None, :]  # the corner column of top[y][x][k]
    top = np.broadcast_to(-z + (X * (2 * z)) // n, (n, n, 4)).astype(np.int32)
    return sc.case(np.zeros((n, n), np.int32), top, False)


def own_shapes():
    """name -> (case, tolerances, bin)"""
    t0 = ((0, 1),)
    shapes = {f"pstrip_{n}": (mc.strip(n), t0, 3) for n in STRIPS}
    shapes["slope_wide"] = (slope(Z_MAX), t0, 1000)
    shapes["slope_narrow"] = (slope(1000), t0, 1000)
    return shapes


OWN_BINS = {"bay": 4, "staircase": 4, "wide": 3, "band": 4, "nested": 25}


def bin_of(name):
    return OWN_BINS.get(name, BINS[zlib.crc32(name.encode()) % len(BINS)])


def all_runs():
    """(name, case, (num, den), bin) of everything the suites run"""
    for name, c, tol in mc.all_runs():
        yield name, c, tol, bin_of(name)
    for name, (c, tols, b) in own_shapes().items():
        for tol in tols:
            yield name, c, tol, b


def _z_of(c, x, y, bin, rng, far=0.1):
    """heights near the pixel's top, a share of them far off"""
    top = np.asarray(c["top"], np.int64)
    t = top[y // bin, x // bin]
    z = (t[:, 0] + t[:, 3]) // 2 + rng.integers(-25, 26, len(x))
    off = rng.random(len(x)) < far
    z = z + np.where(off, rng.integers(2000, 20000, len(x)) * rng.choice((-1, 1), len(x)), 0)
    return np.clip(z, -Z_MAX, Z_MAX)


def tie_points(clean, tri, bin, rng, cap=TIE_CAP):
    """for every triangle edge whose reduced direction in doubled units has two odd components: cell centres (odd in both
    coordinates) that lie exactly on it, as millimetre cells (x, y)"""
    P = np.asarray(clean.sxy, np.int64).reshape(-1, 2)
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3)
    out = set()
    for a, b, c in T[(T != -1).any(axis=1)].tolist():
        for u, v in ((b, c), (c, a), (a, b)):
            dx, dy = (2 * bin * (P[v] - P[u])).tolist()
            g = math.gcd(abs(dx), abs(dy))
            if g == 0 or (dx // g) % 2 == 0 or (dy // g) % 2 == 0:
                continue
            ks = np.arange(1, g, 2)
            for k in (ks if len(ks) <= 40 else rng.choice(ks, 40, replace=False)).tolist():
                px, py = 2 * bin * int(P[u][0]) + k * (dx // g), 2 * bin * int(P[u][1]) + k * (dy // g)
                out.add(((px - 1) // 2, (py - 1) // 2))
    pts = np.array(sorted(out), np.int64).reshape(-1, 2)
    return pts if len(pts) <= cap else pts[np.sort(rng.choice(len(pts), cap, replace=False))]


def cloud(name, c, tol, bin, clean, tri, n_random=None):
    """the seeded cloud of a run: random points over the whole extent, the four corner cells, the centre cell of every pixel
    of a strip, and the tie points; with planes 0 .. N_PLANES - 1 per point and per label"""
    rng = np.random.default_rng(zlib.crc32(f"{name}/{tol[0]}/{tol[1]}".encode()))
    h, w = c["label"].shape
    W, H = w * bin, h * bin
    ntri = max(int(tri.n_triangles), 1)
    nr = int(np.clip(PAIRS // ntri, 32, 1000)) if n_random is None else int(n_random)
    parts = [np.stack([rng.integers(0, W, nr), rng.integers(0, H, nr)], axis=1),
             np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.int64)]
    if name.startswith("pstrip_"):
        parts.append(np.stack([np.arange(w) * bin + bin // 2, np.full(w, bin // 2)], axis=1))
    ties = tie_points(clean, tri, bin, rng)
    parts.append(ties)
    xy = np.concatenate(parts).astype(np.int64)
    z = _z_of(c, xy[:, 0], xy[:, 1], bin, rng)
    nl = int(c["n_labels"])
    return SimpleNamespace(xyz=np.concatenate([xy, z[:, None]], axis=1).astype(np.int32), bin=int(bin),
                           plane_idx=rng.integers(0, N_PLANES, len(xy)).astype(np.int32),
                           label_plane=(np.arange(nl) % N_PLANES).astype(np.int32), clip2=CLIP2, n_ties=len(ties))


def raster_cloud(c):
    """one point per pixel in raster order at bin 1, at the pixel's doubled height halved: the fourth promise"""
    h, w = c["label"].shape
    ys, xs = np.mgrid[0:h, 0:w]
    top = np.asarray(c["top"], np.int64)
    z = np.clip((top[:, :, 0] + top[:, :, 3]) // 2, -Z_MAX, Z_MAX)
    return np.stack([xs.reshape(-1), ys.reshape(-1), z.reshape(-1)], axis=1).astype(np.int32)


def regimes(tri, result, trace):
    """the regimes a run reaches: from the triangles' statuses, the restatement's result and its trace"""
    out = {k for k in ("tie_owned", "tie_not_owned") if trace.get(k, 0) > 0}
    for k, v in (("multi", result.n_multi), ("uncovered", result.n_uncovered), ("long_list", result.max_list > 1),
                 ("empty_pixel", result.n_empty_pixel), ("height_wide", result.n_height_wide),
                 ("height_narrow", result.total_points - result.n_height_wide), ("above", result.total_above),
                 ("below", result.total_below), ("plane_agrees", result.total_plane_points),
                 ("plane_differs", result.total_points - result.total_plane_points)):
        if v > 0:
            out.add(k)
    if trace.get("max_span", 0) > pref.CHUNK:
        out.add("span_over_chunk")
    status = np.asarray(tri.label_status)
    if ((status == tbrute.NO_BRIDGE) | (status == tbrute.STALLED)).any() and result.n_uncovered > 0:
        out.add("failed_label")
    nl = result.n_labels
    if nl == pref.FIG_CAP - 1 and result.points[nl - 1] > 0:
        out.add("labels_below_cap")
    if nl == pref.FIG_CAP and result.points[nl - 1] > 0:
        out.add("labels_at_cap")
    if nl > pref.FIG_CAP and result.points[pref.FIG_CAP:].sum() > 0:
        out.add("labels_above_cap")
    return out
