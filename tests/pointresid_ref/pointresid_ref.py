"""Point residuals, a numpy restatement of the device layout ("Point residuals"): per triangle the pixel rows it
touches, per row the pixel columns that the triangle clipped to the row's band touches, by exact integer floor and ceiling, a
list of slots per pixel, and per point the entries of its pixel's list with the three weights and the tie rule.  The height is
formed as the device forms it: relative to the lowest of the three sz, in int64 where the bit lengths of D and of the largest
height difference prove that it fits, with Python integers elsewhere (n_height_wide).  The implementation's own figures
(n_rows, n_items, max_list, n_empty_pixel) come out as the device counts them.  brute.py is the definition: this file must
equal it."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


brute = _load("pointresid_brute", os.path.join(HERE, "brute.py"))
RangeError, InvalidError, NO_CLIP2 = brute.RangeError, brute.InvalidError, brute.NO_CLIP2

FIG_CAP = 256  # BS_PRESID_FIG_CAP of include/bs_api.h
CHUNK = 256    # BS_PRESID_CHUNK
GRID = 2048    # BS_PRESID_GRID
WORK = ("n_rows", "n_items", "max_list", "n_empty_pixel", "n_height_wide")
DEVICE_FIELDS = brute.FIELDS + WORK  # what the device and the restatement share
BLOCK = 1 << 21  # (point, entry) pairs of one numpy block
I64_MAX = np.iinfo(np.int64).max


def _bits(v):
    """the bit length of every non-negative int64"""
    v = np.asarray(v, np.int64)
    out = np.zeros(v.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (v >> s) > 0
        out += np.where(big, s, 0)
        v = np.where(big, v >> s, v)
    return out + (v > 0)


def lists(clean, tri, width, height):
    """the CSR lists of slots per pixel: (off [h * w + 1], slot [n_items] ascending inside a pixel, n_rows, max_span)"""
    w, h = int(width), int(height)
    P = np.asarray(clean.sxy, np.int64).reshape(-1, 2)
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3)
    slots = np.flatnonzero((T != -1).any(axis=1))
    Tv = T[slots]
    V = P[Tv] if len(Tv) else np.zeros((0, 3, 2), np.int64)  # [slot][corner][x, y]
    # rows
    y0, y1 = np.maximum(V[:, :, 1].min(axis=1), 0), np.minimum(V[:, :, 1].max(axis=1), h)
    rows = np.maximum(y1 - y0, 0) if len(Tv) else np.zeros(0, np.int64)
    n_rows = int(rows.sum())
    rt = np.repeat(np.arange(len(Tv)), rows)  # the triangle of every row item
    ry = y0[rt] + (np.arange(n_rows) - np.repeat(np.cumsum(rows) - rows, rows))
    # spans: the vertices in the band y .. y + 1 and the crossings of its two lines
    lo, hi = np.full(n_rows, I64_MAX, np.int64), np.full(n_rows, -I64_MAX, np.int64)
    R = V[rt]
    for i in range(3):
        U = R[:, i]
        inside = (U[:, 1] >= ry) & (U[:, 1] <= ry + 1)
        lo = np.where(inside, np.minimum(lo, U[:, 0]), lo)
        hi = np.where(inside, np.maximum(hi, U[:, 0]), hi)
    for i, j in ((1, 2), (2, 0), (0, 1)):
        U, W = R[:, i], R[:, j]
        for k in (ry, ry + 1):
            cross = ((U[:, 1] < k) & (W[:, 1] > k)) | ((U[:, 1] > k) & (W[:, 1] < k))
            den, num = W[:, 1] - U[:, 1], (W[:, 0] - U[:, 0]) * (k - U[:, 1])
            num, den = np.where(den < 0, -num, num), np.where(cross, np.abs(den), 1)
            q = num // den
            lo = np.where(cross, np.minimum(lo, U[:, 0] + q), lo)
            hi = np.where(cross, np.maximum(hi, U[:, 0] + q + (num - q * den != 0)), hi)
    has = lo != I64_MAX
    f, l = np.maximum(np.where(has, lo, 0), 0), np.minimum(np.where(has, hi, 0) - 1, w - 1)
    span = np.where(has & (f <= l), l - f + 1, 0)
    n_items = int(span.sum())
    k = np.repeat(np.arange(n_rows), span)
    x = f[k] + (np.arange(n_items) - np.repeat(np.cumsum(span) - span, span))
    pix = ry[k] * w + x
    slot = slots[rt[k]]
    order = np.lexsort((slot, pix))
    off = np.zeros(h * w + 1, np.int64)
    np.cumsum(np.bincount(pix, minlength=h * w), out=off[1:])
    return off, slot[order], n_rows, (int(span.max()) if n_rows else 0)


def point_residuals(clean, tri, n_labels, width, height, xyz, bin, plane_idx=None, label_plane=None, clip2=NO_CLIP2, trace=None):
    """as brute.point_residuals; trace: a dict that receives the ties met (a weight of 0 on a list entry whose other weights
    do not exclude it: owned, not owned) and max_span"""
    nl, w, h, bin = int(n_labels), int(width), int(height), int(bin)
    X = brute.check_arguments(w, h, xyz, bin, plane_idx, label_plane, clip2)
    n = len(X)
    P2 = 2 * bin * np.asarray(clean.sxy, np.int64).reshape(-1, 2)
    Z = np.asarray(clean.sz, np.int64).reshape(-1)
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3)
    toff = np.asarray(tri.tri_offset, np.int64)
    valid = (T != -1).any(axis=1)
    if (np.abs(Z[T[valid]]) >= 1 << 24).any():
        raise RangeError("sz")
    off, slot, n_rows, max_span = lists(clean, tri, w, h)
    if len(slot) >= (1 << 31) - 1:
        raise RangeError("list entries")
    pix = (X[:, 1] // bin) * w + X[:, 0] // bin
    lo, cnt = off[pix], off[pix + 1] - off[pix]
    win = np.full(n, I64_MAX, np.int64)
    cover = np.zeros(n, np.int64)
    ties = [0, 0]
    ends = np.cumsum(cnt)
    i0 = 0
    while i0 < n:  # a block of points at a time
        i1 = max(int(np.searchsorted(ends, (ends[i0 - 1] if i0 else 0) + BLOCK, side="right")), i0 + 1)
        c = cnt[i0:i1]
        pt = np.repeat(np.arange(i0, i1), c)
        t = slot[lo[pt] + (np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c))]
        A, B, C = P2[T[t, 0]], P2[T[t, 1]], P2[T[t, 2]]
        wa, wb, wc, inside = _weights(A, B, C, 2 * X[pt, 0] + 1, 2 * X[pt, 1] + 1)
        tie = ((wa == 0) | (wb == 0) | (wc == 0)) & (wa >= 0) & (wb >= 0) & (wc >= 0)
        ties[0] += int((tie & inside).sum())
        ties[1] += int((tie & ~inside).sum())
        np.minimum.at(win, pt[inside], t[inside])
        np.add.at(cover, pt[inside], 1)
        i0 = i1
    covered = np.flatnonzero(win != I64_MAX)
    wt = win[covered]
    M = np.full(n, -1, np.int64)
    M[covered] = np.searchsorted(toff, wt, side="right") - 1
    r2 = np.full(n, brute.INT32_MIN, np.int64)
    a, b, c = T[wt, 0], T[wt, 1], T[wt, 2]
    wa, wb, wc, inside = _weights(P2[a], P2[b], P2[c], 2 * X[covered, 0] + 1, 2 * X[covered, 1] + 1)
    assert inside.all()
    D = wa + wb + wc
    zm = np.minimum(Z[a], np.minimum(Z[b], Z[c]))
    da, db, dc = Z[a] - zm, Z[b] - zm, Z[c] - zm
    wide = _bits(D) + _bits(np.maximum(da, np.maximum(db, dc))) > 60
    q = np.zeros(len(covered), np.int64)
    nar = ~wide
    N = wa[nar] * da[nar] + wb[nar] * db[nar] + wc[nar] * dc[nar]
    q[nar] = (4 * N + D[nar]) // (2 * D[nar])
    for k in np.flatnonzero(wide).tolist():
        Nk = int(wa[k]) * int(da[k]) + int(wb[k]) * int(db[k]) + int(wc[k]) * int(dc[k])
        q[k] = (4 * Nk + int(D[k])) // (2 * int(D[k]))
    r2[covered] = 2 * X[covered, 2] - (2 * zm + q)
    fig, tot = _figures(nl, M, r2, cover, plane_idx, label_plane, int(clip2))
    if trace is not None:
        trace.update(tie_owned=ties[0], tie_not_owned=ties[1], max_span=max_span)
    i32 = lambda v: v.astype(np.int32)  # noqa: E731
    return brute.SimpleNamespace(width=w, height=h, n_labels=nl, bin=bin, clip2=int(clip2), n_points=n, n_triangles=len(T),
                                 label=i32(M), r2=i32(r2), cover=i32(cover), **fig, **tot, n_rows=n_rows, n_items=len(slot),
                                 max_list=int((off[1:] - off[:-1]).max()), n_empty_pixel=int((cnt == 0).sum()),
                                 n_height_wide=int(wide.sum()))


def _weights(A, B, C, px, py):
    """A, B, C: doubled positions [n][2]; the three weights and the coverage by the tie rule"""
    ax, ay, bx, by, cx, cy = A[:, 0] - px, A[:, 1] - py, B[:, 0] - px, B[:, 1] - py, C[:, 0] - px, C[:, 1] - py
    wa, wb, wc = bx * cy - by * cx, cx * ay - cy * ax, ax * by - ay * bx
    own = lambda w, up: (w > 0) | ((w == 0) & up)  # noqa: E731
    return wa, wb, wc, own(wa, C[:, 1] > B[:, 1]) & own(wb, A[:, 1] > C[:, 1]) & own(wc, B[:, 1] > A[:, 1])


def _figures(nl, M, r2, cover, plane_idx, label_plane, clip2):
    """the per-label figures by numpy (every sum stays far inside int64)"""
    def count(idx, v=None):
        out = np.zeros(nl, np.int64)
        np.add.at(out, idx, 1 if v is None else v)
        return out

    cov = M >= 0
    inl = cov & (r2 >= -clip2) & (r2 <= clip2)
    e = np.abs(r2[inl])
    mx = np.zeros(nl, np.int64)
    np.maximum.at(mx, M[inl], e)
    if plane_idx is None:
        agrees = np.zeros(len(M), bool)
    else:
        lp = np.asarray(label_plane, np.int64).reshape(-1)
        agrees = cov & (np.asarray(plane_idx, np.int64).reshape(-1) == lp[np.where(cov, M, 0)] if nl else cov & False)
    fig = dict(points=count(M[cov]), multi=count(M[cov & (cover > 1)]), above=count(M[cov & (r2 > clip2)]),
               below=count(M[cov & (r2 < -clip2)]), in_points=count(M[inl]), sum_r2=count(M[inl], r2[inl]),
               sum_abs_r2=count(M[inl], e), max_abs_r2=mx, sq_lo=count(M[inl], (e * e) & 0xFFFFFFFF),
               sq_hi=count(M[inl], (e * e) >> 32), plane_points=count(M[agrees]), plane_in=count(M[agrees & inl]))
    tot = {"total_" + k: int(fig[k].sum()) for k in brute.PER_LABEL if k not in ("multi", "max_abs_r2")}
    tot.update(max_abs_r2_all=int(mx.max()) if nl else 0, n_uncovered=int((~cov).sum()), n_multi=int(fig["multi"].sum()))
    return fig, tot


def same(a, b, fields=DEVICE_FIELDS):
    return brute.same(a, b, fields)
