"""Model raster, the definition (include/bs_api.h, "model raster") with Python integers: every pixel against every triangle.
Nothing here knows about rows, spans or boxes."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

INT32_MIN = -(1 << 31)
PER_LABEL = ("pixels", "model_pixels", "kept", "multi", "err_pixels", "sum_abs_e2", "max_abs_e2", "sq_lo", "sq_hi")
TOTALS = ("total_pixels", "total_model_pixels", "total_kept", "total_err_pixels", "total_sum_abs_e2", "max_abs_e2_all",
          "total_sq_lo", "total_sq_hi", "n_uncovered", "n_spill", "n_moved", "n_multi", "sum_cover")
IMAGES = ("model", "cover", "mz2")
FIELDS = ("width", "height", "n_labels", "n_triangles") + TOTALS + PER_LABEL + IMAGES


class RangeError(ValueError):
    """BS_ERR_RANGE of the stage"""


def _owns(w, up):
    return w > 0 or (w == 0 and up)


def _prepare(clean, tri, n_labels):
    """the triangle slots that are not -1 as tuples of Python integers, in slot order, and the label of every slot"""
    P = np.asarray(clean.sxy, np.int64).reshape(-1, 2).tolist()
    Z = np.asarray(clean.sz, np.int64).reshape(-1).tolist()
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3).tolist()
    toff = np.asarray(tri.tri_offset, np.int64).tolist()
    slot_label = [-1] * len(T)
    for l in range(int(n_labels)):
        for t in range(toff[l], toff[l + 1]):
            slot_label[t] = l
    tris = []
    for t, (a, b, c) in enumerate(T):
        if a == -1 and b == -1 and c == -1:
            continue
        if max(abs(Z[a]), abs(Z[b]), abs(Z[c])) >= 1 << 24:
            raise RangeError("sz")
        tris.append((t, 2 * P[a][0], 2 * P[a][1], 2 * P[b][0], 2 * P[b][1], 2 * P[c][0], 2 * P[c][1], Z[a], Z[b], Z[c]))
    return tris, slot_label, len(T)


def _pixel(tris, slot_label, x, y):
    """(cover, M, mz2) of pixel (x, y): its centre against every triangle"""
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
    assert D > 0 and abs(4 * N + D) < 1 << 61
    return n, slot_label[t], (4 * N + D) // (2 * D)


def sample(clean, tri, n_labels, pixels):
    """[(cover, M, mz2)] of the listed pixels (x, y) alone: for images too large for model_raster"""
    tris, slot_label, _ = _prepare(clean, tri, n_labels)
    return [_pixel(tris, slot_label, x, y) for x, y in pixels]


def model_raster(clean, tri, label, top, n_labels):
    """clean: sxy, sz of the clean vertices; tri: tri [n][3] and tri_offset [n_labels + 1]; label [h][w]; top [h][w][4]"""
    label = np.asarray(label)
    h, w = label.shape
    nl = int(n_labels)
    tris, slot_label, n_slots = _prepare(clean, tri, nl)
    lab = label.tolist()
    tp = np.asarray(top, np.int64)
    model = np.full((h, w), -1, np.int32)
    cover = np.zeros((h, w), np.int32)
    mz2 = np.full((h, w), INT32_MIN, np.int32)
    fig = {k: [0] * nl for k in PER_LABEL}
    tot = dict.fromkeys(TOTALS, 0)
    for y in range(h):
        for x in range(w):
            L = lab[y][x] if 0 <= lab[y][x] < nl else -1
            n, M, z2 = _pixel(tris, slot_label, x, y)
            if M >= 0:
                model[y, x], mz2[y, x] = M, z2
            cover[y, x] = n
            tot["sum_cover"] += n
            tot["n_multi"] += n > 1
            if L >= 0:
                fig["pixels"][L] += 1
            tot["n_uncovered"] += L >= 0 and M < 0
            tot["n_spill"] += L < 0 and M >= 0
            tot["n_moved"] += L >= 0 and M >= 0 and L != M
            if M >= 0:
                fig["model_pixels"][M] += 1
                fig["kept"][M] += L == M
                fig["multi"][M] += n > 1
                if L >= 0:
                    s = int(tp[y, x, 0]) + int(tp[y, x, 3])
                    if abs(s) >= 1 << 25:
                        raise RangeError("top")
                    e = abs(int(mz2[y, x]) - s)
                    fig["err_pixels"][M] += 1
                    fig["sum_abs_e2"][M] += e
                    fig["max_abs_e2"][M] = max(fig["max_abs_e2"][M], e)
                    fig["sq_lo"][M] += (e * e) & 0xFFFFFFFF
                    fig["sq_hi"][M] += (e * e) >> 32
    return finish(w, h, nl, n_slots, model, cover, mz2, {k: np.array(v, np.int64).reshape(nl) for k, v in fig.items()}, tot)


def finish(w, h, nl, ntri, model, cover, mz2, fig, tot, **more):
    for k in ("pixels", "model_pixels", "kept", "err_pixels", "sum_abs_e2", "sq_lo", "sq_hi"):
        tot["total_" + k] = int(fig[k].sum())
    tot["max_abs_e2_all"] = int(fig["max_abs_e2"].max()) if nl else 0
    return SimpleNamespace(width=w, height=h, n_labels=nl, n_triangles=ntri, model=model, cover=cover, mz2=mz2,
                           **fig, **{k: int(v) for k, v in tot.items()}, **more)


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


def check_promises(r, label, statuses=None, tolerance_zero=False):
    """the three promises of the definition, with Python integers"""
    kept = int(r.kept.sum())
    assert int(r.pixels.sum()) == kept + r.n_moved + r.n_uncovered
    assert int(r.model_pixels.sum()) == kept + r.n_moved + r.n_spill
    if tolerance_zero and statuses is not None and all(int(s) in (0, 3) for s in statuses):
        lab = np.asarray(label)
        L = np.where((lab >= 0) & (lab < r.n_labels), lab, -1)
        assert np.array_equal(r.model, L) and np.array_equal(r.cover, (L >= 0).astype(np.int32))
