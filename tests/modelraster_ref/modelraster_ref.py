"""Model raster, a numpy restatement of the device layout ("Model raster"): per triangle the rows of its box, per
row the pixels whose centres lie between the two edge crossings, by exact integer ceiling and floor, per candidate pixel the
three weights with the tie rule.  All triangles go through numpy at once, a block of pixel items at a time, so that the
600 x 600 noise of the GPU test and a 5 M point scene take seconds; the implementation's own figures (n_rows, n_items,
n_empty_spans, max_span) come out of it as the device counts them.  brute.py is the definition and boxwise.py its
restatement per triangle over its box, which shares no row or span with this file: this file must equal both."""
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


brute = _load("modelraster_brute", os.path.join(HERE, "brute.py"))
RangeError = brute.RangeError

FIG_CAP = 512  # BS_MRASTER_FIG_CAP of include/bs_api.h
CHUNK = 256    # BS_MRASTER_CHUNK
WORK = ("n_rows", "n_items", "n_empty_spans", "max_span")
DEVICE_FIELDS = brute.FIELDS + WORK  # what the device and the restatement share
BLOCK = 1 << 22  # pixel items of one numpy block
I64_MAX = np.iinfo(np.int64).max


def _weights(A, B, C, px, py):
    """A, B, C: doubled positions [n][2]; the three weights and the coverage by the tie rule"""
    ax, ay, bx, by, cx, cy = A[:, 0] - px, A[:, 1] - py, B[:, 0] - px, B[:, 1] - py, C[:, 0] - px, C[:, 1] - py
    wa, wb, wc = bx * cy - by * cx, cx * ay - cy * ax, ax * by - ay * bx
    own = lambda w, up: (w > 0) | ((w == 0) & up)  # noqa: E731
    return wa, wb, wc, own(wa, C[:, 1] > B[:, 1]) & own(wb, A[:, 1] > C[:, 1]) & own(wc, B[:, 1] > A[:, 1])


def model_raster(clean, tri, label, top, n_labels, trace=None):
    """as brute.model_raster; trace: a dict that receives the ties met (a weight of 0 on a candidate pixel whose other
    weights do not exclude it: owned, not owned)"""
    label = np.asarray(label)
    h, w = label.shape
    nl = int(n_labels)
    P2 = 2 * np.asarray(clean.sxy, np.int64).reshape(-1, 2)
    Z = np.asarray(clean.sz, np.int64).reshape(-1)
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3)
    toff = np.asarray(tri.tri_offset, np.int64)
    slots = np.flatnonzero((T != -1).any(axis=1))
    Tv = T[slots]
    if (np.abs(Z[Tv]) >= 1 << 24).any():
        raise RangeError("sz")
    win = np.full(h * w, I64_MAX, np.int64)
    cover = np.zeros(h * w, np.int64)
    ties = [0, 0]
    # rows
    Y = P2[Tv][:, :, 1] // 2
    y0, y1 = np.maximum(Y.min(axis=1), 0), np.minimum(Y.max(axis=1), h)
    rows = np.maximum(y1 - y0, 0) if len(Tv) else np.zeros(0, np.int64)
    n_rows = int(rows.sum())
    rt = np.repeat(np.arange(len(Tv)), rows)  # the triangle of every row item
    ry = y0[rt] + (np.arange(n_rows) - np.repeat(np.cumsum(rows) - rows, rows))
    # spans
    yc = 2 * ry + 1
    xlo, xhi = np.full(n_rows, I64_MAX, np.int64), np.full(n_rows, -I64_MAX, np.int64)
    for i, j in ((1, 2), (2, 0), (0, 1)):
        U, V = P2[Tv[rt, i]], P2[Tv[rt, j]]
        cross = (U[:, 1] < yc) != (V[:, 1] < yc)
        den, num = V[:, 1] - U[:, 1], (V[:, 0] - U[:, 0]) * (yc - U[:, 1])
        num, den = np.where(den < 0, -num, num), np.where(cross, np.abs(den), 1)
        n, d = (U[:, 0] - 1) * den + num, 2 * den  # the crossing is at X = U.x + num / den; a centre is at 2 x + 1
        q = n // d
        xlo = np.where(cross, np.minimum(xlo, q + (n - q * d != 0)), xlo)
        xhi = np.where(cross, np.maximum(xhi, q), xhi)
    has = xlo != I64_MAX
    f, l = np.maximum(np.where(has, xlo, 0), 0), np.minimum(np.where(has, xhi, 0), w - 1)
    span = np.where(has & (f <= l), l - f + 1, 0)
    n_items = int(span.sum())
    # pixel items, a block of rows at a time
    ends = np.cumsum(span)
    r = 0
    while r < n_rows:
        r1 = max(int(np.searchsorted(ends, (ends[r - 1] if r else 0) + BLOCK, side="right")), r + 1)
        sp = span[r:r1]
        k = np.repeat(np.arange(r, r1), sp)
        x = f[k] + (np.arange(int(sp.sum())) - np.repeat(np.cumsum(sp) - sp, sp))
        t = rt[k]
        wa, wb, wc, inside = _weights(P2[Tv[t, 0]], P2[Tv[t, 1]], P2[Tv[t, 2]], 2 * x + 1, 2 * ry[k] + 1)
        tie = ((wa == 0) | (wb == 0) | (wc == 0)) & (wa >= 0) & (wb >= 0) & (wc >= 0)
        ties[0] += int((tie & inside).sum())
        ties[1] += int((tie & ~inside).sum())
        p = (ry[k] * w + x)[inside]
        np.minimum.at(win, p, slots[t[inside]])
        np.add.at(cover, p, 1)
        r = r1
    # figures
    covered = np.flatnonzero(win != I64_MAX)
    wt = win[covered]
    M = np.full(h * w, -1, np.int64)
    M[covered] = np.searchsorted(toff, wt, side="right") - 1
    mz2 = np.full(h * w, brute.INT32_MIN, np.int64)
    a, b, c = T[wt, 0], T[wt, 1], T[wt, 2]
    wa, wb, wc, inside = _weights(P2[a], P2[b], P2[c], 2 * (covered % w) + 1, 2 * (covered // w) + 1)
    assert inside.all()
    D, N = wa + wb + wc, wa * Z[a] + wb * Z[b] + wc * Z[c]
    mz2[covered] = (4 * N + D) // (2 * D)
    L = label.reshape(-1).astype(np.int64)
    L = np.where((L >= 0) & (L < nl), L, -1)
    both = np.flatnonzero((L >= 0) & (M >= 0))
    tp = np.asarray(top, np.int64).reshape(-1, 4)[both]
    s = tp[:, 0] + tp[:, 3]
    if (np.abs(s) >= 1 << 25).any():
        raise RangeError("top")
    e = np.abs(mz2[both] - s)

    def count(idx, v=None):
        out = np.zeros(nl, np.int64)
        np.add.at(out, idx, 1 if v is None else v)
        return out

    mx = np.zeros(nl, np.int64)
    np.maximum.at(mx, M[both], e)
    fig = dict(pixels=count(L[L >= 0]), model_pixels=count(M[M >= 0]), kept=count(M[(M >= 0) & (L == M)]),
               multi=count(M[(M >= 0) & (cover > 1)]), err_pixels=count(M[both]), sum_abs_e2=count(M[both], e), max_abs_e2=mx,
               sq_lo=count(M[both], (e * e) & 0xFFFFFFFF), sq_hi=count(M[both], (e * e) >> 32))
    tot = dict.fromkeys(brute.TOTALS, 0)
    tot.update(n_uncovered=((L >= 0) & (M < 0)).sum(), n_spill=((L < 0) & (M >= 0)).sum(),
               n_moved=((L >= 0) & (M >= 0) & (L != M)).sum(), n_multi=(cover > 1).sum(), sum_cover=cover.sum())
    if trace is not None:
        trace.update(tie_owned=ties[0], tie_not_owned=ties[1])
    img = lambda v: v.reshape(h, w).astype(np.int32)  # noqa: E731
    return brute.finish(w, h, nl, len(T), img(M), img(cover), img(mz2), fig, tot, n_rows=n_rows, n_items=n_items,
                        n_empty_spans=int((span == 0).sum()), max_span=int(span.max()) if n_rows else 0)


def same(a, b, fields=DEVICE_FIELDS):
    return brute.same(a, b, fields)
