"""Point residuals, the definition (include/bs_api.h, "point residuals") with Python integers: every point against every
triangle.  Nothing here knows about rows, spans, lists or the way the device forms the height."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

INT32_MIN = -(1 << 31)
NO_CLIP2 = (1 << 31) - 1
PER_LABEL = ("points", "multi", "above", "below", "in_points", "sum_r2", "sum_abs_r2", "max_abs_r2", "sq_lo", "sq_hi",
             "plane_points", "plane_in")
TOTALS = ("total_points", "total_above", "total_below", "total_in_points", "total_sum_r2", "total_sum_abs_r2", "max_abs_r2_all",
          "total_sq_lo", "total_sq_hi", "total_plane_points", "total_plane_in", "n_uncovered", "n_multi")
ARRAYS = ("label", "r2", "cover")
FIELDS = ("width", "height", "n_labels", "bin", "clip2", "n_points", "n_triangles") + TOTALS + PER_LABEL + ARRAYS


class RangeError(ValueError):
    """BS_ERR_RANGE of the stage"""


class InvalidError(ValueError):
    """BS_ERR_INVALID of the stage"""


def _owns(w, up):
    return w > 0 or (w == 0 and up)


def check_arguments(width, height, xyz, bin, plane_idx, label_plane, clip2):
    """the errors of the definition that need no triangle"""
    if xyz is None or len(xyz) < 1 or bin < 1 or clip2 < 0 or (plane_idx is None) != (label_plane is None):
        raise InvalidError("arguments")
    if len(xyz) >= 1 << 29 or width * bin > 1 << 24 or height * bin > 1 << 24:
        raise RangeError("points or extent")
    P = np.asarray(xyz, np.int64).reshape(-1, 3)
    if (P[:, :2] < 0).any() or (P[:, 0] // bin >= width).any() or (P[:, 1] // bin >= height).any():
        raise RangeError("a point outside the image")
    if (np.abs(P[:, 2]) >= 1 << 24).any():
        raise RangeError("z")
    return P


def _prepare(clean, tri, n_labels, bin):
    """the triangle slots that are not -1 as tuples of Python integers in doubled millimetres, in slot order, and the label of
    every slot"""
    P = np.asarray(clean.sxy, np.int64).reshape(-1, 2).tolist()
    Z = np.asarray(clean.sz, np.int64).reshape(-1).tolist()
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3).tolist()
    toff = np.asarray(tri.tri_offset, np.int64).tolist()
    slot_label = [-1] * len(T)
    for l in range(int(n_labels)):
        for t in range(toff[l], toff[l + 1]):
            slot_label[t] = l
    s = 2 * int(bin)
    tris = []
    for t, (a, b, c) in enumerate(T):
        if a == -1 and b == -1 and c == -1:
            continue
        if max(abs(Z[a]), abs(Z[b]), abs(Z[c])) >= 1 << 24:
            raise RangeError("sz")
        tris.append((t, s * P[a][0], s * P[a][1], s * P[b][0], s * P[b][1], s * P[c][0], s * P[c][1], Z[a], Z[b], Z[c]))
    return tris, slot_label, len(T)


def _point(tris, slot_label, x, y, z):
    """(cover, M, r2) of the point: the centre of its millimetre cell against every triangle"""
    px, py = 2 * x + 1, 2 * y + 1
    n, win = 0, None
    for rec in tris:
        t, ax, ay, bx, by, cx, cy, za, zb, zc = rec
        wa = (bx - px) * (cy - py) - (by - py) * (cx - px)
        if not _owns(wa, cy > by):
            continue
        wb = (cx - px) * (ay - py) - (cy - py) * (ax - px)
        if not _owns(wb, ay > cy):
            continue
        wc = (ax - px) * (by - py) - (ay - py) * (bx - px)
        if not _owns(wc, by > ay):
            continue
        n += 1
        if win is None:  # (the slots come in ascending order)
            win = (rec, wa, wb, wc)
    if win is None:
        return n, -1, INT32_MIN
    (t, *_, za, zb, zc), wa, wb, wc = win
    D = wa + wb + wc
    N = wa * za + wb * zb + wc * zc
    assert D > 0
    return n, slot_label[t], 2 * z - (4 * N + D) // (2 * D)


def sample(clean, tri, n_labels, bin, points):
    """[(cover, M, r2)] of the listed points (x, y, z) alone"""
    tris, slot_label, _ = _prepare(clean, tri, n_labels, bin)
    return [_point(tris, slot_label, int(x), int(y), int(z)) for x, y, z in points]


def figures(nl, label, r2, cover, plane_idx, label_plane, clip2):
    """the per-label figures and the totals of the three per-point arrays, with Python integers"""
    fig = {k: [0] * nl for k in PER_LABEL}
    tot = dict.fromkeys(TOTALS, 0)
    pl = None if plane_idx is None else np.asarray(plane_idx).reshape(-1).tolist()
    lp = None if label_plane is None else np.asarray(label_plane).reshape(-1).tolist()
    for i, (M, r, n) in enumerate(zip(np.asarray(label).tolist(), np.asarray(r2).tolist(), np.asarray(cover).tolist())):
        if M < 0:
            tot["n_uncovered"] += 1
            continue
        fig["points"][M] += 1
        fig["multi"][M] += n > 1
        inlier = -clip2 <= r <= clip2
        fig["above"][M] += r > clip2
        fig["below"][M] += r < -clip2
        agrees = pl is not None and pl[i] == lp[M]
        fig["plane_points"][M] += agrees
        fig["plane_in"][M] += agrees and inlier
        if inlier:
            e = abs(r)
            fig["in_points"][M] += 1
            fig["sum_r2"][M] += r
            fig["sum_abs_r2"][M] += e
            fig["max_abs_r2"][M] = max(fig["max_abs_r2"][M], e)
            fig["sq_lo"][M] += (e * e) & 0xFFFFFFFF
            fig["sq_hi"][M] += (e * e) >> 32
    for k in PER_LABEL:
        if k not in ("multi", "max_abs_r2", "points"):
            tot["total_" + k] = sum(fig[k])
    tot["total_points"] = sum(fig["points"])
    tot["n_multi"] = sum(fig["multi"])
    tot["max_abs_r2_all"] = max(fig["max_abs_r2"], default=0)
    return {k: np.array(v, np.int64).reshape(nl) for k, v in fig.items()}, tot


def point_residuals(clean, tri, n_labels, width, height, xyz, bin, plane_idx=None, label_plane=None, clip2=NO_CLIP2):
    """clean: sxy, sz of the clean vertices; tri: tri [n][3] and tri_offset [n_labels + 1]; width, height: the image of the
    count; xyz [n][3] millimetres"""
    nl = int(n_labels)
    P = check_arguments(width, height, xyz, bin, plane_idx, label_plane, clip2)
    tris, slot_label, n_slots = _prepare(clean, tri, nl, bin)
    got = [_point(tris, slot_label, x, y, z) for x, y, z in P.tolist()]
    cover, label, r2 = (np.array([g[k] for g in got], np.int32) for k in range(3))
    fig, tot = figures(nl, label, r2, cover, plane_idx, label_plane, clip2)
    return SimpleNamespace(width=width, height=height, n_labels=nl, bin=int(bin), clip2=int(clip2), n_points=len(P),
                           n_triangles=n_slots, label=label, r2=r2, cover=cover, **fig, **tot)


def same(a, b, fields=FIELDS):
    """None, or the first field in which a and b differ"""
    for k in fields:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            if x is None or y is None or np.shape(x) != np.shape(y) or not np.array_equal(x, y):
                return k
        elif int(x) != int(y):
            return k
    return None


def check_promises(r, label_image=None, statuses=None, tolerance_zero=False, xyz=None):
    """the first three promises of the definition, with Python integers"""
    assert r.n_points == int(r.points.sum()) + r.n_uncovered
    assert np.array_equal(r.points, r.in_points + r.above + r.below)
    if tolerance_zero and statuses is not None and all(int(s) in (0, 3) for s in statuses):
        lab = np.asarray(label_image)
        P = np.asarray(xyz, np.int64).reshape(-1, 3)
        L = lab[P[:, 1] // r.bin, P[:, 0] // r.bin]
        assert np.array_equal(r.label, np.where((L >= 0) & (L < r.n_labels), L, -1))
        return True
    return False
