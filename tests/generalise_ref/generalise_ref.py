"""numpy restatement of the roof generalisation (include/bs_api.h, "roof generalisation"): every evaluation is
solid_ref.tops, facet_ref.roof_facets and facet_ref.kinds on the current image; the targets are one maximum per facet over
the candidate list, the chain ends come from pointer jumping.  tests/generalise_ref/brute.py is the per-pixel form it must
equal."""
from __future__ import annotations

import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "solid_ref"))
sys.path.insert(0, os.path.join(HERE, "..", "facet_ref"))
import facet_ref as fr  # noqa: E402
import solid_ref as sr  # noqa: E402


def _load_brute():
    """tests/generalise_ref/brute.py under a name of its own (other reference directories have a brute.py too)"""
    if "generalise_brute" not in sys.modules:
        spec = importlib.util.spec_from_file_location("generalise_brute", os.path.join(HERE, "brute.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["generalise_brute"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["generalise_brute"]


brute = _load_brute()
NAMES, SCALARS, ARRAYS = brute.NAMES, brute.SCALARS, brute.ARRAYS
ORDER_TOP = 2 ** 30 - 1


def evaluate(bmap, R, top, min_pixels, merge_flat, step_tol, bend_tol):
    """one evaluation of R: the facets of facet_ref, the kinds, and per facet target (-1: stays), by_flat, end, links"""
    rf = fr.roof_facets(bmap, R, top)
    nf = rf.n_facets
    kind = fr.kinds(rf, step_tol, bend_tol)
    pixels, plane = rf.facet_pixels.astype(np.int64), rf.facet_plane.astype(np.int64)
    order = np.empty(nf, np.int64)
    order[np.lexsort((np.arange(nf), -pixels))] = np.arange(nf)  # 0 = the highest rank
    best = np.zeros(nf, np.int64)
    if rf.n_edges:
        lo, hi = rf.edge_facet[:, 0].astype(np.int64), rf.edge_facet[:, 1].astype(np.int64)
        up = order[hi] < order[lo]
        f, g = np.where(up, lo, hi), np.where(up, hi, lo)
        by_flat = (kind == 0) & bool(merge_flat)
        ok = (plane[g] > 0) & ((pixels[f] < min_pixels) | by_flat)
        key = (rf.edge_length.astype(np.int64) << 32) | ((ORDER_TOP - order[g]) << 1) | by_flat
        np.maximum.at(best, f[ok], key[ok])
    by_rank = np.argsort(order)
    moves = best != 0
    target = np.where(moves, by_rank[np.where(moves, ORDER_TOP - ((best & 0xFFFFFFFF) >> 1), 0)], -1) if nf else np.zeros(0, np.int64)
    end, links = np.where(moves, target, np.arange(nf)), moves.astype(np.int64)
    while True:
        nxt = end[end]
        if np.array_equal(nxt, end):
            break
        links, end = links + links[end], nxt
    return SimpleNamespace(rf=rf, n_flat=int((kind == 0).sum()), n_small=int((pixels < min_pixels).sum()), moves=moves,
                           by_flat=moves & ((best & 1) == 1), target=target, end=end, links=links, kind=kind, top=top)


def generalise(bmap, roof, n_buildings, normal, center, z_min, z_max, bin, base_z, flat, min_pixels=0, merge_flat=False,
               step_tol=200, bend_tol=0, max_rounds=64):
    bmap = np.asarray(bmap, np.int32)
    R0 = np.asarray(roof, np.int32)
    R = R0.copy()
    n_planes = len(np.asarray(z_min).reshape(-1))
    evals, tops = [], []
    rounds, converged = 0, 0
    r = 1
    while True:
        top = sr.tops(bmap, R, normal, center, z_min, z_max, bin, base_z, flat)
        ev = evaluate(bmap, R, top, min_pixels, merge_flat, step_tol, bend_tol)
        tops.append(top)
        evals.append(ev)
        if not ev.moves.any():
            converged = 1
            break
        if r > max_rounds:
            break
        newp = np.where(ev.moves, ev.rf.facet_plane[ev.end], 0)
        inb = ev.rf.facet >= 0
        p = np.zeros(R.shape, np.int64)
        p[inb] = newp[ev.rf.facet[inb]]
        R = np.where(p > 0, p, R).astype(np.int32)
        rounds = r
        r += 1
    out = SimpleNamespace(roof=R, rounds=rounds, converged=converged, evals=evals)  # (evals: for tests/generalise_ref/cases.py)
    for tag, ev in (("in", evals[0]), ("out", evals[-1])):
        setattr(out, "n_facets_" + tag, ev.rf.n_facets)
        setattr(out, "n_edges_" + tag, ev.rf.n_edges)
        setattr(out, "n_flat_" + tag, ev.n_flat)
        setattr(out, "n_small_" + tag, ev.n_small)
        setattr(out, "building_facets_" + tag, np.bincount(ev.rf.facet_building, minlength=n_buildings).astype(np.int64))
    out.eval_facets = np.asarray([e.rf.n_facets for e in evals], np.int64)
    out.eval_movers = np.asarray([e.moves.sum() for e in evals], np.int64)
    out.eval_movers_flat = np.asarray([e.by_flat.sum() for e in evals], np.int64)
    out.eval_movers_small = out.eval_movers - out.eval_movers_flat
    out.eval_longest_chain = np.asarray([e.links.max() if len(e.links) else 0 for e in evals], np.int64)
    inb = bmap >= 0
    c = bmap[inb]
    p0, p1 = np.maximum(R0[inb], 0), np.maximum(R[inb], 0)
    out.plane_pixels_in = np.bincount(p0, minlength=n_planes + 1).astype(np.int64)
    out.plane_pixels_out = np.bincount(p1, minlength=n_planes + 1).astype(np.int64)
    chg = R0[inb] != R[inb]
    d = np.abs(tops[-1].astype(np.int64) - tops[0].astype(np.int64))[inb]
    out.building_pixels_changed = np.bincount(c, weights=chg, minlength=n_buildings).astype(np.int64)
    out.building_sum_abs_dtop = fr._sum(c, d.sum(1), n_buildings)
    out.building_max_abs_dtop = np.maximum(fr._max(c, d.max(1), n_buildings), 0) if len(c) else np.zeros(n_buildings, np.int64)
    out.pixels_changed = int(chg.sum())
    out.pixels_roofed = int(((p0 == 0) & (p1 > 0)).sum())
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
