"""Model raster, the definition restated per triangle over its box (include/bs_api.h, "model raster"): int64 numpy, one
triangle at a time, every pixel of the triangle's bounding box against the three weights.  Nothing here knows about rows,
spans, crossings or work items, and the figures are counted from the finished images alone: it is the affordable form of
brute.py, whole on every run, and shares no step with modelraster_ref.py but the weights' formula."""
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


def model_raster(clean, tri, label, top, n_labels):
    """as brute.model_raster"""
    label = np.asarray(label)
    h, w = label.shape
    nl = int(n_labels)
    P = np.asarray(clean.sxy, np.int64).reshape(-1, 2)
    Z = np.asarray(clean.sz, np.int64).reshape(-1)
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3)
    toff = np.asarray(tri.tri_offset, np.int64)
    model = np.full((h, w), -1, np.int64)
    cover = np.zeros((h, w), np.int64)
    mz2 = np.full((h, w), brute.INT32_MIN, np.int64)
    slot_label = np.repeat(np.arange(nl), np.diff(toff))
    for t in range(len(T)):  # ascending: the first slot to cover a pixel keeps it
        a, b, c = T[t].tolist()
        if a == -1 and b == -1 and c == -1:
            continue
        if max(abs(int(Z[a])), abs(int(Z[b])), abs(int(Z[c]))) >= 1 << 24:
            raise brute.RangeError("sz")
        (ax, ay), (bx, by), (cx, cy) = P[a].tolist(), P[b].tolist(), P[c].tolist()
        x0, x1 = max(min(ax, bx, cx), 0), min(max(ax, bx, cx), w)
        y0, y1 = max(min(ay, by, cy), 0), min(max(ay, by, cy), h)
        if x0 >= x1 or y0 >= y1:
            continue
        px = 2 * np.arange(x0, x1, dtype=np.int64)[None, :] + 1
        py = 2 * np.arange(y0, y1, dtype=np.int64)[:, None] + 1
        wa = (2 * bx - px) * (2 * cy - py) - (2 * by - py) * (2 * cx - px)
        wb = (2 * cx - px) * (2 * ay - py) - (2 * cy - py) * (2 * ax - px)
        wc = (2 * ax - px) * (2 * by - py) - (2 * ay - py) * (2 * bx - px)
        inside = ((wa >= 0) if cy > by else (wa > 0)) & ((wb >= 0) if ay > cy else (wb > 0)) & ((wc >= 0) if by > ay else (wc > 0))
        if not inside.any():
            continue
        box = (slice(y0, y1), slice(x0, x1))
        first = inside & (cover[box] == 0)
        cover[box] += inside
        D = wa + wb + wc
        N = wa * int(Z[a]) + wb * int(Z[b]) + wc * int(Z[c])
        model[box] = np.where(first, slot_label[t], model[box])
        mz2[box] = np.where(first, (4 * N + D) // np.where(first, 2 * D, 1), mz2[box])
    L = np.where((label >= 0) & (label < nl), label, -1).astype(np.int64)
    both = (L >= 0) & (model >= 0)
    tp = np.asarray(top, np.int64)
    s = tp[..., 0] + tp[..., 3]
    if (np.abs(s[both]) >= 1 << 25).any():
        raise brute.RangeError("top")
    e = np.where(both, np.abs(mz2 - s), 0)
    fig = {k: np.zeros(nl, np.int64) for k in brute.PER_LABEL}
    for l in np.union1d(L[L >= 0], model[model >= 0]).tolist():  # (a label on no pixel keeps its zeros)
        m = model == l
        el = e[m & both]
        fig["pixels"][l] = (L == l).sum()
        fig["model_pixels"][l] = m.sum()
        fig["kept"][l] = (m & (L == l)).sum()
        fig["multi"][l] = (m & (cover > 1)).sum()
        fig["err_pixels"][l] = len(el)
        fig["sum_abs_e2"][l] = el.sum()
        fig["max_abs_e2"][l] = el.max() if len(el) else 0
        fig["sq_lo"][l] = ((el * el) & 0xFFFFFFFF).sum()
        fig["sq_hi"][l] = ((el * el) >> 32).sum()
    tot = dict.fromkeys(brute.TOTALS, 0)
    tot.update(n_uncovered=((L >= 0) & (model < 0)).sum(), n_spill=((L < 0) & (model >= 0)).sum(),
               n_moved=(both & (L != model)).sum(), n_multi=(cover > 1).sum(), sum_cover=cover.sum())
    i32 = lambda v: v.astype(np.int32)  # noqa: E731
    return brute.finish(w, h, nl, len(T), i32(model), i32(cover), i32(mz2), fig, tot)
