"""numpy restatement of the roof facets and their edges (include/bs_api.h, "roof facets"), vectorised over the image so that
a million pixels take about a second: connected components over the equal-class 4-links, renumbered by first pixel, and
the per-edge figures by np.unique over the facet pairs.  tests/facet_ref/brute.py is the per-pixel form it must equal."""
from __future__ import annotations

import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components


def _load_brute():
    """tests/facet_ref/brute.py under a name of its own (tests/solid_ref has a brute.py too)"""
    if "facet_brute" not in sys.modules:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "brute.py")
        spec = importlib.util.spec_from_file_location("facet_brute", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["facet_brute"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["facet_brute"]


brute = _load_brute()

I32_MIN, I32_MAX = brute.I32_MIN, brute.I32_MAX
NAMES = (("facet",) + tuple("facet_" + k for k, _ in brute.FACET_FIELDS) + tuple("edge_" + k for k, _ in brute.EDGE_FIELDS) +
         brute.TOTALS)


def classes(bmap, roof):
    """(building << 32) | plane per pixel, -1 outside every building"""
    bmap, roof = np.asarray(bmap, np.int64), np.asarray(roof, np.int64)
    return np.where(bmap >= 0, (bmap << 32) | np.maximum(roof, 0), -1)


def components(cls, keep_h=None, keep_v=None):
    """component number per pixel over the 4-links between equal classes >= 0 (keep_h / keep_v: masks over the horizontal
    and vertical links that count); pixels outside stay alone"""
    h, w = cls.shape
    idx = np.arange(h * w).reshape(h, w)
    lh = (cls[:, :-1] == cls[:, 1:]) & (cls[:, :-1] >= 0)
    lv = (cls[:-1, :] == cls[1:, :]) & (cls[:-1, :] >= 0)
    if keep_h is not None:
        lh &= keep_h
    if keep_v is not None:
        lv &= keep_v
    a = np.concatenate([idx[:, :-1][lh], idx[:-1, :][lv]])
    b = np.concatenate([idx[:, 1:][lh], idx[1:, :][lv]])
    g = coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(h * w, h * w))
    return connected_components(g, directed=False)[1].reshape(h, w)


def label(bmap, roof):
    """facet int64 [height][width]: components renumbered by ascending first pixel, -1 outside"""
    cls = classes(bmap, roof)
    comp = components(cls)
    inb = cls >= 0
    facet = np.full(cls.shape, -1, np.int64)
    if inb.any():
        lab = comp[inb]  # raster order
        uniq, first = np.unique(lab, return_index=True)
        rank = np.empty(len(uniq), np.int64)
        rank[np.argsort(first)] = np.arange(len(uniq))
        facet[inb] = rank[np.searchsorted(uniq, lab)]
    return facet


def _sum(idx, val, n):
    out = np.zeros(n, np.int64)
    np.add.at(out, idx, np.asarray(val, np.int64))
    return out


def _min(idx, val, n):
    out = np.full(n, I32_MAX, np.int64)
    np.minimum.at(out, idx, val)
    return out


def _max(idx, val, n):
    out = np.full(n, I32_MIN, np.int64)
    np.maximum.at(out, idx, val)
    return out


def border_edges(bmap, facet, top):
    """every border edge in ascending (y, x, direction): dict of arrays y, x, d, fa, fb and the heights of the definition"""
    bmap, top = np.asarray(bmap, np.int64), np.asarray(top, np.int64)
    parts = []
    for d in (0, 1):
        A = (slice(None), slice(None, -1)) if d == 0 else (slice(None, -1), slice(None))
        B = (slice(None), slice(1, None)) if d == 0 else (slice(1, None), slice(None))
        is_border = (bmap[A] >= 0) & (bmap[A] == bmap[B]) & (facet[A] != facet[B])
        y, x = np.nonzero(is_border)
        TA, TB = top[A][is_border], top[B][is_border]
        if d == 0:
            a_s, a_e, b_s, b_e = TA[:, 1], TA[:, 3], TB[:, 0], TB[:, 2]
            s_a, s_b = (TA[:, 1] + TA[:, 3]) - (TA[:, 0] + TA[:, 2]), (TB[:, 1] + TB[:, 3]) - (TB[:, 0] + TB[:, 2])
            sx, sy = x + 1, y
        else:
            a_s, a_e, b_s, b_e = TA[:, 2], TA[:, 3], TB[:, 0], TB[:, 1]
            s_a, s_b = (TA[:, 2] + TA[:, 3]) - (TA[:, 0] + TA[:, 1]), (TB[:, 2] + TB[:, 3]) - (TB[:, 0] + TB[:, 1])
            sx, sy = x, y + 1
        parts.append(dict(y=y, x=x, d=np.full(len(y), d), fa=facet[A][is_border], fb=facet[B][is_border], c=bmap[A][is_border],
                          a_s=a_s, a_e=a_e, b_s=b_s, b_e=b_e, bend=s_a - s_b, sx=sx, sy=sy, ex=x + 1, ey=y + 1))
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    w = bmap.shape[1]
    order = np.argsort((out["y"] * w + out["x"]) * 2 + out["d"], kind="stable")
    return {k: v[order] for k, v in out.items()}


def roof_facets(bmap, roof, top):
    bmap, roof, top = np.asarray(bmap, np.int64), np.asarray(roof, np.int64), np.asarray(top, np.int64)
    h, w = bmap.shape
    facet = label(bmap, roof)
    out = SimpleNamespace(facet=facet.astype(np.int32))
    inb = bmap >= 0
    ys, xs = np.nonzero(inb)
    f = facet[ys, xs]
    nf = int(f.max()) + 1 if len(f) else 0
    _, first = np.unique(f, return_index=True)
    T = top[ys, xs]
    pm = np.full((h + 2, w + 2), -2, np.int64)
    pm[1:-1, 1:-1] = np.where(inb, bmap, -1)
    pf = np.full((h + 2, w + 2), -1, np.int64)
    pf[1:-1, 1:-1] = facet
    inner, outer = np.zeros(len(f), np.int64), np.zeros(len(f), np.int64)
    for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        same = pm[ys + 1 + dy, xs + 1 + dx] == bmap[ys, xs]
        outer += ~same
        inner += same & (pf[ys + 1 + dy, xs + 1 + dx] != f)
    fig = dict(building=bmap[ys, xs][first], plane=np.maximum(roof[ys, xs][first], 0), start_xy=np.stack([xs[first], ys[first]], 1),
               pixels=np.bincount(f, minlength=nf),
               bbox=np.stack([_min(f, xs, nf), _min(f, ys, nf), _max(f, xs, nf), _max(f, ys, nf)], 1),
               inner_edges=_sum(f, inner, nf), outer_edges=_sum(f, outer, nf), top_min=_min(f, T.min(1), nf),
               top_max=_max(f, T.max(1), nf), top_sum=_sum(f, T.sum(1), nf))
    for name, dt in brute.FACET_FIELDS:
        shape = (nf, brute.WIDTH[name]) if name in brute.WIDTH else (nf,)
        setattr(out, "facet_" + name, np.asarray(fig[name]).astype(dt).reshape(shape))
    b = border_edges(bmap, facet, top)
    lo, hi = np.minimum(b["fa"], b["fb"]), np.maximum(b["fa"], b["fb"])
    key, first, e = np.unique(lo * max(nf, 1) + hi, return_index=True, return_inverse=True)
    e = e.reshape(-1)
    ne = len(key)
    ds, de = b["a_s"] - b["b_s"], b["a_e"] - b["b_e"]
    sign = np.where(b["fa"] > b["fb"], 1, -1)
    zs = np.stack([b["a_s"], b["a_e"], b["b_s"], b["b_e"]], 1)
    edge = dict(facet=np.stack([lo[first], hi[first]], 1), building=b["c"][first], length=np.bincount(e, minlength=ne),
                n_dir0=_sum(e, b["d"] == 0, ne), n_step=_sum(e, (ds != 0) | (de != 0), ne),
                step_abs_sum=_sum(e, np.abs(ds) + np.abs(de), ne),
                step_abs_max=np.maximum(_max(e, np.maximum(np.abs(ds), np.abs(de)), ne), 0), rise_sum=_sum(e, sign * (ds + de), ne),
                bend_sum=_sum(e, b["bend"], ne), z_min=_min(e, zs.min(1), ne), z_max=_max(e, zs.max(1), ne),
                bbox=np.stack([_min(e, b["sx"], ne), _min(e, b["sy"], ne), _max(e, b["ex"], ne), _max(e, b["ey"], ne)], 1))
    for name, dt in brute.EDGE_FIELDS:
        shape = (ne, brute.WIDTH[name]) if name in brute.WIDTH else (ne,)
        setattr(out, "edge_" + name, np.asarray(edge[name]).astype(dt).reshape(shape))
    out.n_facets, out.n_edges, out.n_pixels, out.n_border = nf, ne, len(f), len(e)
    return out


def same(a, b, names=NAMES):
    """the first name in which two results differ, or None"""
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(y, np.ndarray):
            if not (isinstance(x, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)):
                return k
        elif int(x) != int(y):
            return k
    return None


def kinds(rf, step_tol, bend_tol):
    """bs_roof_edge_kinds: uint8 [n_edges]"""
    ln, st, bd = (np.asarray(getattr(rf, k), np.int64) for k in ("edge_length", "edge_step_abs_sum", "edge_bend_sum"))
    return np.where(st > 2 * step_tol * ln, 3, np.where(bd > bend_tol * ln, 1, np.where(bd < -bend_tol * ln, 2, 0))).astype(np.uint8)


def obj_text(rf, bmap, top, bin, kind, origin=None):
    """the file of bs_roof_edges_write_obj as bytes"""
    o = np.zeros(3, np.int64) if origin is None else np.asarray(origin, np.int64)
    facet = np.asarray(rf.facet, np.int64)
    b = border_edges(bmap, facet, top)
    nf = max(int(rf.n_facets), 1)
    pairs = np.asarray(rf.edge_facet, np.int64).reshape(-1, 2)
    e = np.searchsorted(pairs[:, 0] * nf + pairs[:, 1], np.minimum(b["fa"], b["fb"]) * nf + np.maximum(b["fa"], b["fb"]))
    order = np.argsort(e, kind="stable")
    rows = np.stack([b["sx"] * bin + o[0], b["sy"] * bin + o[1], np.maximum(b["a_s"], b["b_s"]) + o[2], b["ex"] * bin + o[0],
                     b["ey"] * bin + o[1], np.maximum(b["a_e"], b["b_e"]) + o[2]], 1)[order].tolist()
    eo = e[order].tolist()
    out = [f"# roof edges: {len(pairs)} edges, {len(eo)} segments\n"]
    at = 0
    for k in range(len(pairs)):
        out.append(f"g edge_{k}_{brute.KIND_NAMES[int(kind[k])]}\n")
        while at < len(eo) and eo[at] == k:
            r = rows[at]
            out.append(f"v {r[0]} {r[1]} {r[2]}\nv {r[3]} {r[4]} {r[5]}\nl {2 * at + 1} {2 * at + 2}\n")
            at += 1
    return "".join(out).encode()
