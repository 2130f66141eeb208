"""The device pass of the oriented boxes (buildingsegment_amd/csrc/bs_hull.hip) restated in numpy, array operation for
kernel: the candidates in ascending half-edge order, the two seeds per label, the QuickHull rounds with their 64-bit bids
(distance << 32 | candidate, the highest wins), the sort into walk order, the strictness pass and the boxes.  Its result must
equal brute.py's; its layout figures (n_candidates, rounds, max_live) are what the device must report.  It starts from the
labelled pixels (pixel_hulls) and lays them out in an image without the empty rows and columns between them (squeeze), so a
few pixels in a large image cost what the pixels cost."""
from __future__ import annotations

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


brute = _load("hull_brute", os.path.join(HERE, "brute.py"))
orf = _load("outline_ref", os.path.join(HERE, "..", "outline_ref", "outline_ref.py"))
ROUND_BATCH = 4
CORNER_SHIFT = 14  # corner index = (y << 14) | x, box-relative, both <= 16383


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def squeeze(xs, ys, labs, width, height):
    """(small, cols, rows): the image of the listed pixels without its empty rows and columns, except one after every
    occupied one (so what did not touch still does not touch); cols[x], rows[y] are the places of the small image's columns
    and rows in the large one.  The occupied pixels keep their order and their neighbours, hence the half-edges theirs."""
    cols = np.union1d(xs, xs[xs + 1 < width] + 1) if len(xs) else np.zeros(1, np.int64)
    rows = np.union1d(ys, ys[ys + 1 < height] + 1) if len(ys) else np.zeros(1, np.int64)
    small = np.full((len(rows), len(cols)), -1, np.int64)
    small[np.searchsorted(rows, ys), np.searchsorted(cols, xs)] = labs
    return small, cols, rows


def candidates(xs, ys, labs, width, height, n_labels):
    """(label, X, Y) of every candidate in ascending half-edge order, and box / pixels2 / status per label"""
    label, cols, rows = squeeze(xs, ys, labs, width, height)
    h, w = label.shape
    box = np.zeros((n_labels, 4), np.int64)
    pixels2 = np.zeros(n_labels, np.int64)
    status = np.full(n_labels, brute.EMPTY, np.int64)
    none = np.zeros(0, np.int64)
    flags, base, hnum, x, y, k = orf.half_edges(label)
    if len(hnum) == 0:
        return none, none, none, box, pixels2, status
    tr = {}
    o = orf.outlines(label, None, n_labels, trace=tr)
    np.add.at(pixels2, o.ring_label, o.ring_area2)
    for l in range(n_labels):
        rb = o.ring_bbox[(o.ring_label == l) & (o.ring_area2 > 0)].astype(np.int64)
        if len(rb):
            box[l] = (cols[rb[:, 0].min()], rows[rb[:, 1].min()], cols[rb[:, 2].max() - 1] + 1, rows[rb[:, 3].max() - 1] + 1)
            big = box[l, 2] - box[l, 0] > brute.MAX_SIDE or box[l, 3] - box[l, 1] > brute.MAX_SIDE
            status[l] = brute.TOO_LARGE if big else brute.OK
    leader = tr["leader"]
    sx, sy = x + orf.SX[k], y + orf.SY[k]
    k1 = (k + 1) % 4
    ring_area = np.zeros(len(hnum), np.int64)
    np.add.at(ring_area, leader, sx * (y + orf.SY[k1]) - (x + orf.SX[k1]) * sy)
    lab = label[y, x]
    cand = ((flags[y * w + x] >> ((k + 3) % 4)) & 1 == 1) & (ring_area[leader] > 0) & (status[lab] == brute.OK)
    return lab[cand], (cols[x] + orf.SX[k])[cand], (rows[y] + orf.SY[k])[cand], box, pixels2, status


def label_hulls(label, n_labels=None):
    """from the image: its labelled pixels (np.nonzero), then pixel_hulls"""
    label = np.asarray(label)
    n_labels = max(int(label.max()) + 1, 0) if n_labels is None else int(n_labels)
    ys, xs = np.nonzero(label >= 0)
    return pixel_hulls(xs, ys, label[ys, xs], label.shape[1], label.shape[0], n_labels)


def pixel_hulls(xs, ys, labs, width, height, n_labels):
    """the restatement from the list of labelled pixels (x, y, label) of a width x height image, in any order"""
    xs, ys, labs = (np.asarray(v, np.int64).ravel() for v in (xs, ys, labs))
    clab, X, Y, box, pixels2, status = candidates(xs, ys, labs, width, height, n_labels)
    nc = len(clab)
    r = brute.label_hulls(np.full((1, 1), -1), n_labels)  # (the zeroed result)
    r.width, r.image_height = int(width), int(height)
    r.box[:], r.pixels2[:], r.status[:] = box, pixels2, status
    r.n_ok, r.n_empty, r.n_too_large = (int((status == s).sum()) for s in (brute.OK, brute.EMPTY, brute.TOO_LARGE))
    r.info = dict(n_candidates=nc, rounds=0, max_live=0)
    if nc == 0:
        return r
    rx, ry = X - box[clab, 0], Y - box[clab, 1]
    ck = (ry << CORNER_SHIFT) | rx
    ids = np.arange(nc)
    key = (ck << 32) | ids
    smin, smax = np.full(n_labels, np.iinfo(np.int64).max), np.zeros(n_labels, np.int64)
    np.minimum.at(smin, clab, key)
    np.maximum.at(smax, clab, key)
    a, b = (smin & 0xffffffff)[clab], (smax & 0xffffffff)[clab]
    nextv = np.full(nc, -1, np.int64)
    ok = np.nonzero(status == brute.OK)[0]
    nextv[smin[ok] & 0xffffffff], nextv[smax[ok] & 0xffffffff] = smax[ok] & 0xffffffff, smin[ok] & 0xffffffff
    # the first assignment
    o = _orient(rx[a], ry[a], rx[b], ry[b], rx, ry)
    edge = np.where(o < 0, a, np.where(o > 0, b, -1))
    edge[(ids == a) | (ids == b)] = -2
    chain = (o > 0).astype(np.int64)
    best = np.zeros(nc, np.int64)
    live = edge >= 0
    np.maximum.at(best, edge[live], (np.abs(o[live]) << 32) | ids[live])
    lives = [int(live.sum())]
    while True:
        for _ in range(ROUND_BATCH):
            nxt = np.zeros(nc, np.int64)
            c = np.nonzero(edge >= 0)[0]
            ea = edge[c]
            f = best[ea] & 0xffffffff
            eb = nextv[ea]
            d1 = -_orient(rx[ea], ry[ea], rx[f], ry[f], rx[c], ry[c])
            d2 = -_orient(rx[f], ry[f], rx[eb], ry[eb], rx[c], ry[c])
            win = f == c
            to_a, to_f = ~win & (d1 > 0), ~win & (d1 <= 0) & (d2 > 0)
            assert not (to_a & (d2 > 0)).any()
            edge[c[to_f]] = f[to_f]
            edge[c[~win & ~to_a & ~to_f]] = -1
            np.maximum.at(nxt, ea[to_a], (d1[to_a] << 32) | c[to_a])
            np.maximum.at(nxt, f[to_f], (d2[to_f] << 32) | c[to_f])
            lives.append(int(to_a.sum() + to_f.sum()))
            wc, wa = c[win], ea[win]  # apply
            nextv[wc] = nextv[wa]
            nextv[wa] = wc
            edge[wc] = -2
            best = nxt
        if lives[-1] == 0:
            break
    r.info.update(rounds=sum(v > 0 for v in lives), max_live=max(lives))
    # order: (label, chain, +-corner), then the strict vertices
    hv = np.nonzero(edge == -2)[0]
    skey = (clab[hv] << 32) | np.where(chain[hv] == 1, 0x80000000 | (0x7fffffff - ck[hv]), ck[hv])
    hv = hv[np.argsort(skey, kind="stable")]
    lo = np.searchsorted(clab[hv], np.arange(n_labels + 1))
    i = np.arange(len(hv))
    first, last = lo[clab[hv]], lo[clab[hv] + 1]
    prev, nxt_i = hv[np.where(i == first, last - 1, i - 1)], hv[np.where(i + 1 == last, first, i + 1)]
    turn = _orient(rx[prev], ry[prev], rx[hv], ry[hv], rx[nxt_i], ry[nxt_i])
    assert (turn >= 0).all()
    keep = turn > 0
    spos = np.cumsum(keep) - keep
    r.hull_offset[:] = np.concatenate([spos, [int(keep.sum())]])[lo]
    r.n_hull[:] = np.diff(r.hull_offset)
    r.hull_xy = np.stack([X[hv[keep]], Y[hv[keep]]], axis=1).astype(np.int32)
    r.n_hull_vertices = len(r.hull_xy)
    # boxes: every edge against every vertex of its label, the least by exact comparison, the lowest edge on a tie
    for l in ok:
        ring = [(int(p[0]), int(p[1])) for p in r.hull_xy[r.hull_offset[l]:r.hull_offset[l + 1]]]
        bi, bb = None, None
        for e in range(len(ring)):
            cur = brute.edge_box(ring, e)
            if bb is None or cur[4] * bb[0] < bb[4] * cur[0]:
                bi, bb = e, cur
        r.hull_area2[l], r.best_edge[l], r.dir[l] = brute.area2(ring), bi, bb[5]
        r.len2[l], r.a_min[l], r.a_max[l], r.c_max[l], r.area_num[l] = bb[:5]
    return r
