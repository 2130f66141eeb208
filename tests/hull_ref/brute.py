"""The oriented boxes (include/bs_api.h, "oriented boxes") straight from the definition, in Python integers: the corners of
every pixel of a label, a monotone chain with strict turns, every hull edge's rectangle compared as fractions, and the
corner rounding.  Nothing here knows how the device pass is laid out."""
from __future__ import annotations

from fractions import Fraction
from types import SimpleNamespace

import numpy as np

MAX_SIDE = 16383
OK, EMPTY, TOO_LARGE = 0, 1, 2
PER_LABEL = ("status", "box", "pixels2", "n_hull", "hull_offset", "hull_area2", "best_edge", "dir", "len2", "a_min", "a_max",
             "c_max", "area_num")
TOTALS = ("n_hull_vertices", "n_ok", "n_empty", "n_too_large")


def orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def corners(label, l):
    """C(l): the lattice corners of all pixels of label l, as a set of (X, Y) in Python integers"""
    ys, xs = np.nonzero(np.asarray(label) == l)
    out = set()
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        out.update(zip((xs + dx).tolist(), (ys + dy).tolist()))
    return out


def hull(points):
    """the strict vertices of the convex hull, positive shoelace sum in (X, Y), from the lowest (Y, X)"""
    pts = sorted(points)
    if len(pts) < 3:
        return pts

    def chain(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and orient(out[-2], out[-1], p) <= 0:
                out.pop()
            out.append(p)
        return out[:-1]

    ring = chain(pts) + chain(reversed(pts))
    start = min(range(len(ring)), key=lambda i: (ring[i][1], ring[i][0]))
    return ring[start:] + ring[:start]


def area2(ring):
    return sum(ring[i][0] * ring[(i + 1) % len(ring)][1] - ring[(i + 1) % len(ring)][0] * ring[i][1] for i in range(len(ring)))


def edge_box(ring, i):
    """(len2, a_min, a_max, c_max, area_num, d) of the rectangle on hull edge i"""
    s, e = ring[i], ring[(i + 1) % len(ring)]
    d = (e[0] - s[0], e[1] - s[1])
    a = [(p[0] - s[0]) * d[0] + (p[1] - s[1]) * d[1] for p in ring]
    c = [orient(s, e, p) for p in ring]
    assert min(c) >= 0
    return d[0] * d[0] + d[1] * d[1], min(a), max(a), max(c), (max(a) - min(a)) * max(c), d


def best_box(ring):
    """(i, edge_box(i)) of the least area, the lowest i on a tie"""
    best = None
    for i in range(len(ring)):
        b = edge_box(ring, i)
        if best is None or Fraction(b[4], b[0]) < Fraction(best[1][4], best[1][0]):
            best = (i, b)
    return best


def edge_products(ring):
    """[(area_num_i, len2_i)] of every hull edge: what the comparison area_num_i * len2_j < area_num_j * len2_i sees"""
    return [(b[4], b[0]) for b in (edge_box(ring, i) for i in range(len(ring)))]


def ring_of(r, l):
    """the hull of label l as a list of (X, Y) in Python integers"""
    return [(int(p[0]), int(p[1])) for p in r.hull_xy[int(r.hull_offset[l]):int(r.hull_offset[l + 1])]]


def label_hulls(label, n_labels=None):
    """from the image: its labelled pixels (np.nonzero), then pixel_hulls"""
    label = np.asarray(label)
    n_labels = max(int(label.max()) + 1, 0) if n_labels is None else int(n_labels)
    ys, xs = np.nonzero(label >= 0)
    return pixel_hulls(xs, ys, label[ys, xs], label.shape[1], label.shape[0], n_labels)


def pixel_hulls(xs, ys, labs, width, height, n_labels):
    """the definition from the list of labelled pixels (x, y, label) of a width x height image, in any order"""
    xs, ys, labs = (np.asarray(v, np.int64).ravel() for v in (xs, ys, labs))
    r = SimpleNamespace(width=int(width), image_height=int(height), n_labels=n_labels)
    for k in PER_LABEL:
        cols = {"box": 4, "dir": 2}.get(k)
        n = n_labels + (k == "hull_offset")
        r.__dict__[k] = np.zeros((n, cols) if cols else n, np.int32 if k in ("status", "box", "best_edge", "dir") else np.int64)
    xy = []
    order = np.argsort(labs, kind="stable")  # the pixels of every label, grouped once
    lo = np.searchsorted(labs[order], np.arange(n_labels + 1))
    for l in range(n_labels):
        r.hull_offset[l] = len(xy)
        pix = order[lo[l]:lo[l + 1]]
        pts = set()
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            pts.update(zip((xs[pix] + dx).tolist(), (ys[pix] + dy).tolist()))
        if not pts:
            r.status[l] = EMPTY
            continue
        cx, cy = [p[0] for p in pts], [p[1] for p in pts]
        r.box[l] = (min(cx), min(cy), max(cx), max(cy))
        r.pixels2[l] = 2 * len(pix)
        if max(cx) - min(cx) > MAX_SIDE or max(cy) - min(cy) > MAX_SIDE:
            r.status[l] = TOO_LARGE
            continue
        ring = hull(pts)
        i, (len2, a0, a1, c, num, d) = best_box(ring)
        r.n_hull[l], r.hull_area2[l], r.best_edge[l], r.dir[l] = len(ring), area2(ring), i, d
        r.len2[l], r.a_min[l], r.a_max[l], r.c_max[l], r.area_num[l] = len2, a0, a1, c, num
        xy += ring
    r.hull_offset[n_labels] = len(xy)
    r.hull_xy = np.array(xy, np.int32).reshape(-1, 2)
    r.n_hull_vertices = len(xy)
    r.n_ok, r.n_empty, r.n_too_large = (int((r.status == s).sum()) for s in (OK, EMPTY, TOO_LARGE))
    return r


def same(a, b, layout=()):
    """None if the two results agree in every total, per-label array and hull vertex, else the first name that differs"""
    for k in TOTALS + PER_LABEL + ("hull_xy",) + tuple(layout):
        x, y = (v.info[k] if k in layout and hasattr(v, "info") else getattr(v, k) for v in (a, b))
        if not np.array_equal(np.asarray(x), np.asarray(y)):
            return k
    return None


def round_div(num, den):
    """num / den rounded half away from zero (den > 0)"""
    q = (2 * abs(num) + den) // (2 * den)
    return -q if num < 0 else q


def box_corners(r, l, bin=1, origin=None):
    """[[X, Y]] * 4 of the rectangle of label l: K0, K1, K2, K3 of the header"""
    assert r.status[l] == OK
    ox, oy = (0, 0) if origin is None else (int(origin[0]), int(origin[1]))
    s = [int(v) for v in r.hull_xy[int(r.hull_offset[l]) + int(r.best_edge[l])]]
    dx, dy, len2 = int(r.dir[l][0]), int(r.dir[l][1]), int(r.len2[l])
    a0, a1, c = int(r.a_min[l]), int(r.a_max[l]), int(r.c_max[l])
    num = [(s[0] * len2 + a0 * dx, s[1] * len2 + a0 * dy), (s[0] * len2 + a1 * dx, s[1] * len2 + a1 * dy),
           (s[0] * len2 + a1 * dx - c * dy, s[1] * len2 + a1 * dy + c * dx),
           (s[0] * len2 + a0 * dx - c * dy, s[1] * len2 + a0 * dy + c * dx)]
    return [[round_div(x * bin, len2) + ox, round_div(y * bin, len2) + oy] for x, y in num]


def obj_text(r, bin, origin=None):
    """the bytes of bs_hull_boxes_write_obj"""
    org = [0, 0, 0] if origin is None else [int(v) for v in origin]
    out = [f"# oriented boxes: {r.n_labels} labels, {r.n_ok} ok, {r.n_empty} empty, {r.n_too_large} too large, "
           f"{r.n_hull_vertices} hull vertices"]
    at = 1

    def polyline(n):
        nonlocal at
        out.append("l " + " ".join(str(at + v) for v in range(n)) + f" {at}")
        at += n

    for l in range(r.n_labels):
        if r.status[l] != OK:
            continue
        out.append(f"g label_{l}_hull")
        for v in range(int(r.hull_offset[l]), int(r.hull_offset[l] + r.n_hull[l])):
            out.append(f"v {int(r.hull_xy[v][0]) * bin + org[0]} {int(r.hull_xy[v][1]) * bin + org[1]} {org[2]}")
        polyline(int(r.n_hull[l]))
        out.append(f"g label_{l}_box")
        for x, y in box_corners(r, l, bin, org):
            out.append(f"v {x} {y} {org[2]}")
        polyline(4)
    return "\n".join(out) + "\n"


def identities(r):
    """the identities of the header on every BS_HULL_OK label"""
    for l in np.nonzero(r.status == OK)[0]:
        x0, y0, x1, y1 = (int(v) for v in r.box[l])
        a2, num, len2 = int(r.hull_area2[l]), int(r.area_num[l]), int(r.len2[l])
        assert r.n_hull[l] >= 4 and a2 >= int(r.pixels2[l]) > 0, l
        assert 2 * num >= a2 * len2 and num <= (x1 - x0) * (y1 - y0) * len2, l
        assert r.a_min[l] <= 0 and r.a_max[l] >= len2 and r.c_max[l] > 0, l
        ring = [tuple(int(v) for v in p) for p in r.hull_xy[int(r.hull_offset[l]):int(r.hull_offset[l + 1])]]
        assert ring[0] == min(ring, key=lambda p: (p[1], p[0])) and area2(ring) == a2, l
        assert all(orient(ring[i - 1], ring[i], ring[(i + 1) % len(ring)]) > 0 for i in range(len(ring))), l
        assert any(ring[i][1] == ring[(i + 1) % len(ring)][1] for i in range(len(ring))), l
    for l in np.nonzero(r.status != OK)[0]:
        assert r.n_hull[l] == 0 and r.area_num[l] == 0 and r.hull_area2[l] == 0 and r.len2[l] == 0, l
    assert np.array_equal(np.diff(r.hull_offset), r.n_hull) and r.hull_offset[-1] == r.n_hull_vertices == len(r.hull_xy)
