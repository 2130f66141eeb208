"""Facet outlines by brute force (include/bs_api.h, "facet outlines"): every ring is walked half-edge by half-edge in plain
Python, straight from the definition.  Slow and obvious; tests/outline_ref/outline_ref.py must equal it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

DELTA = ((0, -1), (1, 0), (0, 1), (-1, 0))
START = ((0, 0), (1, 0), (1, 1), (0, 1))  # start corner of side k, relative to the pixel
ZIDX = (0, 1, 3, 2)                       # which of {t00, t10, t01, t11} lies at that corner
FIELDS = ("n_half", "n_rings", "n_vertices", "ring_label", "ring_start", "ring_length", "ring_vertices", "ring_area2",
          "ring_bbox", "ring_offset", "label_ring_offset", "xy", "z")


def pack(n_labels, rings, has_z):
    """rings: (label, h0, length, area2, bbox, [(X, Y, Z)]) in any order -> the result in the listed order"""
    rings = sorted(rings, key=lambda r: (r[0], r[1]))
    nr = len(rings)
    verts = [v for r in rings for v in r[5]]
    lro = np.zeros(n_labels + 1, np.int64)
    for r in rings:
        lro[r[0] + 1] += 1
    return SimpleNamespace(
        n_labels=n_labels, n_half=sum(r[2] for r in rings), n_rings=nr, n_vertices=len(verts),
        ring_label=np.array([r[0] for r in rings], np.int32), ring_start=np.array([r[1] for r in rings], np.int32),
        ring_length=np.array([r[2] for r in rings], np.int64), ring_vertices=np.array([len(r[5]) for r in rings], np.int64),
        ring_area2=np.array([r[3] for r in rings], np.int64), ring_bbox=np.array([r[4] for r in rings], np.int32).reshape(nr, 4),
        ring_offset=np.concatenate([[0], np.cumsum([len(r[5]) for r in rings])]).astype(np.int64),
        label_ring_offset=np.cumsum(lro),
        xy=np.array([v[:2] for v in verts], np.int32).reshape(len(verts), 2),
        z=np.array([v[2] for v in verts], np.int32) if has_z else None)


def outlines(label, top=None, n_labels=None):
    label = np.asarray(label, np.int64)
    h, w = label.shape
    n_labels = max(int(label.max()) + 1, 0) if n_labels is None else n_labels

    def inside(r, p):
        return 0 <= r[0] < w and 0 <= r[1] < h and label[r[1], r[0]] == label[p[1], p[0]]

    def step(p, k):
        return (p[0] + DELTA[k][0], p[1] + DELTA[k][1])

    def succ(p, k):
        p1 = step(p, (k + 1) % 4)
        q = step(p1, k)
        if not inside(p1, p):
            return p, (k + 1) % 4
        if not inside(q, p):
            return p1, k
        return q, (k + 3) % 4

    half = [((x, y), k) for y in range(h) for x in range(w) if label[y, x] >= 0 for k in range(4)
            if not inside(step((x, y), k), (x, y))]
    seen, rings = set(), []
    for p0, k0 in half:  # ascending half-edge number: the first unseen one of a ring is its start
        if (p0, k0) in seen:
            continue
        walk, (p, k) = [], (p0, k0)
        while (p, k) not in seen:
            seen.add((p, k))
            walk.append((p, k))
            p, k = succ(p, k)
        assert (p, k) == (p0, k0)
        area2, xs, ys, verts = 0, [], [], []
        for j, (p, k) in enumerate(walk):
            s = (p[0] + START[k][0], p[1] + START[k][1])
            e = (p[0] + START[(k + 1) % 4][0], p[1] + START[(k + 1) % 4][1])
            area2 += s[0] * e[1] - e[0] * s[1]
            xs += [s[0], e[0]]
            ys += [s[1], e[1]]
            if walk[j - 1][1] != k:  # the predecessor has another side number
                verts.append((s[0], s[1], int(top[p[1]][p[0]][ZIDX[k]]) if top is not None else 0))
        rings.append((int(label[p0[1], p0[0]]), 4 * (p0[1] * w + p0[0]) + k0, len(walk), area2,
                      (min(xs), min(ys), max(xs), max(ys)), verts))
    assert len(seen) == len(half)
    return pack(n_labels, rings, top is not None)


def obj_text(o, bin, origin=None):
    """the OBJ of bs_outlines_write_obj as bytes"""
    org = (0, 0, 0) if origin is None else tuple(int(v) for v in origin)
    lines = [f"# facet outlines: {o.n_labels} labels, {o.n_rings} rings, {o.n_vertices} vertices"]
    for r in range(o.n_rings):
        lab = int(o.ring_label[r])
        lines.append(f"g label_{lab}_ring_{r - int(o.label_ring_offset[lab])}_{'outer' if o.ring_area2[r] > 0 else 'hole'}")
        a, b = int(o.ring_offset[r]), int(o.ring_offset[r + 1])
        for v in range(a, b):
            z = int(o.z[v]) if o.z is not None else 0
            lines.append(f"v {int(o.xy[v, 0]) * bin + org[0]} {int(o.xy[v, 1]) * bin + org[1]} {z + org[2]}")
        lines.append("l " + " ".join(str(v + 1) for v in list(range(a, b)) + [a]))
    return ("\n".join(lines) + "\n").encode()
