"""The ground stage in numpy (include/bs_api.h, "ground"): the separable opening by shifted minima and maxima, whole images at
a time, checked against tests/ground_ref/brute.py; and the per-point rule of the ground model (include/bs_api.h, "ground
model") for the raster, the assignment and the roofs."""
import importlib.util
import os
import sys
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


brute = _load("ground_brute", os.path.join(HERE, "brute.py"))
EMPTY = brute.EMPTY
FIGURES = brute.FIGURES
I32_MIN = -2 ** 31


def params(cell=500, max_radius_mm=12800, slope=(3, 10), dh0=200, dh_max=2500, tol=200, min_height=2000, radius=None):
    """the parameters as a dict; the radii double 1, 2, 4, ... while r * cell <= max_radius_mm unless they are given"""
    if radius is None:
        radius, r = [], 1
        while r * cell <= max_radius_mm and r <= brute.MAX_RADIUS and len(radius) < brute.MAX_STEPS:
            radius.append(r)
            r *= 2
    return dict(cell=int(cell), radius=[int(r) for r in radius], s_num=int(slope[0]), s_den=int(slope[1]), dh0=int(dh0),
                dh_max=int(dh_max), tol=int(tol), min_height=int(min_height))


def _line(a, r, axis, pick, ident):
    """pick over the 2r+1 entries around every entry along axis, clipped; `ident` never wins"""
    out = a.copy()
    n = a.shape[axis]
    for d in range(1, min(r, n - 1) + 1):
        sl_lo = [slice(None)] * 2
        sl_hi = [slice(None)] * 2
        sl_lo[axis], sl_hi[axis] = slice(0, n - d), slice(d, n)
        lo, hi = tuple(sl_lo), tuple(sl_hi)
        out[lo] = pick(out[lo], a[hi])
        out[hi] = pick(out[hi], a[lo])
    return out


def erode(S, r):
    return _line(_line(S, r, 1, np.minimum, EMPTY), r, 0, np.minimum, EMPTY)


def dilate(E, r):
    m = np.where(E == EMPTY, I32_MIN, E)
    m = _line(_line(m, r, 0, np.maximum, I32_MIN), r, 1, np.maximum, I32_MIN)
    return np.where(m == I32_MIN, EMPTY, m)


def ground(xyz, extent, p):
    """SimpleNamespace: width, height, threshold, step_pixels, low, dtm (int32 [h][w]), step (uint8), hag (int32 [n]),
    cls (uint8 [n]) and every name of FIGURES.  Raises the errors of brute.check."""
    w, h = brute.check(xyz, extent, p)
    cell = p["cell"]
    q = np.asarray(xyz, dtype=np.int64)
    if (q[:, :2] < 0).any() or (q[:, 0] // cell >= w).any() or (q[:, 1] // cell >= h).any():
        raise brute.RangeError("xy")
    if (np.abs(q) >= brute.COORD_LIMIT).any():
        raise brute.RangeError("coordinate")
    pix = (q[:, 1] // cell) * w + q[:, 0] // cell
    low = np.full(w * h, EMPTY, np.int64)
    np.minimum.at(low, pix, q[:, 2])
    low = low.reshape(h, w)
    S = low.copy()
    step = np.where(low == EMPTY, 255, 0).astype(np.uint8)
    th = brute.thresholds(p)
    step_pixels = []
    for k, r in enumerate(p["radius"], 1):
        O = dilate(erode(S, r), r)
        hit = (step == 0) & (S != EMPTY) & (S - O > th[k - 1])
        step[hit] = k
        step_pixels.append(int(hit.sum()))
        S = O
    dtm = np.where(step == 0, low, S)
    hag = q[:, 2] - dtm.ravel()[pix]
    st = step.ravel()[pix]
    cls = np.where((st == 0) & (hag <= p["tol"]), 0, np.where(hag >= p["min_height"], 2, 1)).astype(np.uint8)
    have = dtm[dtm != EMPTY]
    out = SimpleNamespace(width=w, height=h, threshold=th, step_pixels=step_pixels, low=low.astype(np.int32),
                          dtm=dtm.astype(np.int32), step=step, hag=hag.astype(np.int32), cls=cls)
    out.n_ground_pixels = int((step == 0).sum())
    out.n_object_pixels = int(((step > 0) & (step < 255)).sum())
    out.n_empty_pixels = int((low == EMPTY).sum())
    out.n_filled_pixels = int(((low == EMPTY) & (dtm != EMPTY)).sum())
    out.n_ground_points, out.n_low_points, out.n_object_points = (int((cls == c).sum()) for c in range(3))
    out.dtm_min = int(have.min()) if len(have) else EMPTY
    out.dtm_max = int(have.max()) if len(have) else I32_MIN
    out.hag_min, out.hag_max = int(hag.min()), int(hag.max())
    out.sum_hag_ground = int(hag[cls == 0].sum())
    return out


def same(a, b):
    """None if the restatement's result a equals the brute force's dict b everywhere, else the name that differs"""
    for k in ("width", "height", "threshold", "step_pixels") + FIGURES:
        if getattr(a, k) != b[k]:
            return k
    for k in ("low", "dtm", "step", "hag", "cls"):
        if not np.array_equal(np.asarray(getattr(a, k), np.int64), np.asarray(b[k], np.int64)):
            return k
    return None


# ---- the ground model: "below ground" per point, and the 2-D branch under it ------------------------------------------------
def ground_th(xyz, bin_height=1000):
    """the scalar threshold of the raster: the lower edge of the height bin that holds the tile's median z"""
    z = np.asarray(xyz)[:, 2].astype(np.int64)
    hist = np.bincount(z // bin_height, minlength=int(z.max()) // bin_height + 1)
    b = int(np.argmax(np.cumsum(hist) > len(z) // 2))
    return float(b * bin_height)


def below(xyz, th, model=None):
    """bool [n]: the point is below ground.  model = None: z < th.  model = (dtm, cell, min_height): z < dtm[pixel] +
    min_height, and z < th for a point whose model pixel is outside the table or EMPTY"""
    q = np.asarray(xyz, dtype=np.int64)
    out = q[:, 2].astype(np.float64) < th
    if model is None:
        return out
    dtm, cell, min_height = model
    dtm = np.asarray(dtm, dtype=np.int64)
    h, w = dtm.shape
    gx, gy = q[:, 0] // cell, q[:, 1] // cell
    inside = (q[:, 0] >= 0) & (q[:, 1] >= 0) & (gx < w) & (gy < h)
    g = np.full(len(q), EMPTY, np.int64)
    g[inside] = dtm[gy[inside], gx[inside]]
    use = g != EMPTY
    out[use] = q[use, 2] < g[use] + min_height
    return out


def splat_mask(xyz, keep, extent, bin=100):
    """uint8 [h][w]: the pixels that a kept point touches with a non-zero bilinear weight -- the mask of the raster's density
    channel at any threshold below 20 (a touched pixel holds log(c + 1) + 20)"""
    q = np.asarray(xyz, dtype=np.int64)[np.asarray(keep)]
    w, h = int(extent[0]) // bin + 2, int(extent[1]) // bin + 2
    m = np.zeros((h, w), np.uint8)
    x, y = q[:, 0] // bin, q[:, 1] // bin
    fx, fy = q[:, 0] % bin != 0, q[:, 1] % bin != 0  # the weight of the far corner is zero on a lattice line
    m[y, x] = 1
    m[y[fx], x[fx] + 1] = 1
    m[y[fy] + 1, x[fy]] = 1
    m[y[fx & fy] + 1, x[fx & fy] + 1] = 1
    return m


def box_scores(bmap, truth):
    """per box of the truth map: the IoU of the building of bmap that matches it best (0.0 without one)"""
    out = []
    for c in range(int(truth.max()) + 1):
        t = truth == c
        best = 0.0
        for b in np.unique(bmap[t & (bmap >= 0)]):
            m = bmap == b
            best = max(best, float((m & t).sum()) / float((m | t).sum()))
        out.append(best)
    return out
