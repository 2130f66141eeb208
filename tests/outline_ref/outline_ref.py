"""Facet outlines (include/bs_api.h, "facet outlines") as the device computes them, restated in numpy: side flags, the
exclusive sum of their popcounts and the compact ids, the successor table, exactly R = ceil(log2 n_half) doubling rounds
for the leaders, the cut in front of the leader, R Wyllie rounds for the suffix counts of vertices, the key sort of the
rings.  tests/outline_ref/brute.py walks the rings instead; the two must be equal."""
from __future__ import annotations

import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np


def _load_brute():
    """tests/outline_ref/brute.py under a name of its own (other reference directories have a brute.py too)"""
    if "outline_brute" not in sys.modules:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "brute.py")
        spec = importlib.util.spec_from_file_location("outline_brute", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["outline_brute"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["outline_brute"]


brute = _load_brute()

DX = np.array([0, 1, 0, -1])
DY = np.array([-1, 0, 1, 0])
SX = np.array([0, 1, 1, 0])  # start corner of side k
SY = np.array([0, 0, 1, 1])
ZIDX = np.array([0, 1, 3, 2])
POP = np.array([bin(v).count("1") for v in range(16)])
END = -1


def rounds_of(n_half):
    """R: the smallest R with 2^R >= n_half"""
    r = 0
    while (1 << r) < n_half:
        r += 1
    return r


def same_label(label, x, y, lab):
    """in(r, p) for arrays of neighbours r = (x, y) and the labels lab of p"""
    h, w = label.shape
    ok = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    return ok & (label[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)] == lab)


def half_edges(label):
    """flags[pixel], base[pixel] and per compact half-edge: its number, x, y, side"""
    h, w = label.shape
    ys, xs = np.mgrid[0:h, 0:w]
    flags = np.zeros((h, w), np.int64)
    for k in range(4):
        flags |= ((label >= 0) & ~same_label(label, xs + DX[k], ys + DY[k], label)).astype(np.int64) << k
    flags = flags.ravel()
    cnt = POP[flags]
    base = np.cumsum(cnt) - cnt
    nz = np.nonzero(flags)[0]
    sub, k = np.nonzero((flags[nz, None] >> np.arange(4)) & 1)  # row-major: ascending half-edge number
    pix = nz[sub]
    return flags, base, 4 * pix + k, pix % w, pix // w, k


def outlines(label, top=None, n_labels=None, trace=None):
    label = np.asarray(label, np.int64)
    h, w = label.shape
    n_labels = max(int(label.max()) + 1, 0) if n_labels is None else n_labels
    flags, base, hnum, x, y, k = half_edges(label)
    n = len(hnum)
    if n == 0:
        return brute.pack(n_labels, [], top is not None)
    lab = label[y, x]

    def compact(px, py, side):
        p = py * w + px
        assert ((flags[p] >> side) & 1).all()
        return base[p] + POP[flags[p] & ((1 << side) - 1)]

    # successor: left turn, straight on, right turn
    k1, k3 = (k + 1) % 4, (k + 3) % 4
    p1x, p1y = x + DX[k1], y + DY[k1]
    qx, qy = p1x + DX[k], p1y + DY[k]
    left = (flags[y * w + x] >> k1 & 1) == 1
    straight = ~left & ~same_label(label, qx, qy, lab)
    tx = np.where(left, x, np.where(straight, p1x, qx))
    ty = np.where(left, y, np.where(straight, p1y, qy))
    tk = np.where(left, k1, np.where(straight, k, k3))
    succ = compact(tx, ty, tk)
    # vertex: the predecessor has another side number
    ax, ay = x + DX[k3], y + DY[k3]
    vert = ((flags[y * w + x] >> k3 & 1) == 1) | same_label(label, ax + DX[k], ay + DY[k], lab)
    # leaders: R doubling rounds, double-buffered
    R = rounds_of(n)
    mn, nxt = np.arange(n), succ.copy()
    for _ in range(R):
        mn, nxt = np.minimum(mn, mn[nxt]), nxt[nxt]
    leader = mn
    # the cut in front of the leader, then R Wyllie rounds: val = the vertices from the element to the tail
    nxt = np.where(succ == leader, END, succ)
    val = vert.astype(np.int64)
    for _ in range(R):
        live = nxt != END
        j = np.where(live, nxt, 0)
        val, nxt = np.where(live, val + val[j], val), np.where(live, nxt[j], END)
    assert (nxt == END).all()
    # rings: leaders flagged and scanned, sorted by (label << 32) | leader
    is_lead = leader == np.arange(n)
    slot_of = np.cumsum(is_lead) - is_lead
    lead = np.nonzero(is_lead)[0]
    order = np.argsort((lab[lead] << 32) | lead, kind="stable")
    inv = np.empty(len(lead), np.int64)
    inv[order] = np.arange(len(lead))
    ring = inv[slot_of[leader]]
    nr = len(lead)
    rv = val[lead][order]
    sx, sy = x + SX[k], y + SY[k]
    ex, ey = x + SX[k1], y + SY[k1]
    length, area2 = np.zeros(nr, np.int64), np.zeros(nr, np.int64)
    np.add.at(length, ring, 1)
    np.add.at(area2, ring, sx * ey - ex * sy)
    bbox = np.empty((nr, 4), np.int64)
    bbox[:, :2], bbox[:, 2:] = 1 << 40, -1
    np.minimum.at(bbox[:, 0], ring, np.minimum(sx, ex))
    np.minimum.at(bbox[:, 1], ring, np.minimum(sy, ey))
    np.maximum.at(bbox[:, 2], ring, np.maximum(sx, ex))
    np.maximum.at(bbox[:, 3], ring, np.maximum(sy, ey))
    offset = np.concatenate([[0], np.cumsum(rv)])
    nv = int(offset[-1])
    # emit: a vertex stands at its ring's offset + (the ring's vertices - its suffix count)
    v = np.nonzero(vert)[0]
    dest = offset[ring[v]] + rv[ring[v]] - val[v]
    xy = np.zeros((nv, 2), np.int32)
    hit = np.zeros(nv, np.int64)
    np.add.at(hit, dest, 1)
    assert (hit == 1).all()
    xy[dest, 0], xy[dest, 1] = sx[v], sy[v]
    z = None
    if top is not None:
        z = np.zeros(nv, np.int32)
        z[dest] = np.asarray(top)[y[v], x[v], ZIDX[k[v]]]
    if trace is not None:
        trace.update(R=R, succ=succ, vert=vert, leader=leader, hnum=hnum)
    rl = lab[lead][order]
    return SimpleNamespace(
        n_labels=n_labels, n_half=n, n_rings=nr, n_vertices=nv, ring_label=rl.astype(np.int32),
        ring_start=hnum[lead][order].astype(np.int32), ring_length=length, ring_vertices=rv.astype(np.int64), ring_area2=area2,
        ring_bbox=bbox.astype(np.int32), ring_offset=offset.astype(np.int64),
        label_ring_offset=np.searchsorted(rl, np.arange(n_labels + 1)).astype(np.int64), xy=xy, z=z)


def same(a, b):
    """None if the two results are equal, else the name of the first field that differs"""
    for f in brute.FIELDS:
        u, v = getattr(a, f), getattr(b, f)
        if (u is None) != (v is None):
            return f
        if u is None:
            continue
        u, v = np.asarray(u), np.asarray(v)
        if u.shape != v.shape or not np.array_equal(u.astype(np.int64), v.astype(np.int64)):
            return f
    return None


def identities(o, label, connected):
    """what every result satisfies; `connected`: every label is one 4-connected component (the (*) identities)"""
    label = np.asarray(label, np.int64)
    assert int(o.ring_length.sum()) == o.n_half and int(o.ring_vertices.sum()) == o.n_vertices == int(o.ring_offset[-1])
    assert np.array_equal(np.diff(o.ring_offset), o.ring_vertices) and o.label_ring_offset[-1] == o.n_rings
    assert ((o.ring_vertices % 2 == 0) & (o.ring_vertices >= 4)).all()
    key = (o.ring_label.astype(np.int64) << 32) | o.ring_start
    assert (np.diff(key) > 0).all()
    pixels = np.bincount(label[label >= 0], minlength=o.n_labels)
    area = np.zeros(o.n_labels, np.int64)
    np.add.at(area, o.ring_label, o.ring_area2)
    assert np.array_equal(area, 2 * pixels)
    assert np.array_equal(np.bincount(o.ring_label, minlength=o.n_labels), np.diff(o.label_ring_offset))
    if connected:
        first = o.label_ring_offset[:-1][np.diff(o.label_ring_offset) > 0]
        pos = np.zeros(o.n_rings, bool)
        pos[first] = True
        assert np.array_equal(o.ring_area2 > 0, pos)
        flat = label.ravel()
        start = np.full(o.n_labels, -1, np.int64)
        idx = np.nonzero(flat >= 0)[0][::-1]
        start[flat[idx]] = idx  # (the last write wins: the first pixel in raster order)
        assert np.array_equal(o.ring_start[first], 4 * start[o.ring_label[first]])
