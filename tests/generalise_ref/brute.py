"""The roof generalisation (include/bs_api.h, "roof generalisation") in plain Python, pixel by pixel: a flood fill for the
facets, a dict of edges, targets followed by a loop.  Only the tops come from tests/solid_ref (the height function is
pinned there).  tests/generalise_ref/generalise_ref.py is the vectorised form that must equal it."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "solid_ref"))
import solid_ref as sr  # noqa: E402

SCALARS = ("rounds", "converged", "n_facets_in", "n_facets_out", "n_edges_in", "n_edges_out", "n_flat_in", "n_flat_out",
           "n_small_in", "n_small_out", "pixels_changed", "pixels_roofed")
EVAL = ("eval_facets", "eval_movers", "eval_movers_small", "eval_movers_flat", "eval_longest_chain")
ARRAYS = EVAL + ("plane_pixels_in", "plane_pixels_out", "building_facets_in", "building_facets_out",
                 "building_pixels_changed", "building_sum_abs_dtop", "building_max_abs_dtop")
NAMES = ("roof",) + SCALARS + ARRAYS


def evaluate(bmap, R, top, min_pixels, merge_flat, step_tol, bend_tol):
    """one evaluation: dict with facet (list of lists), pixels, plane, building, edges {(lo, hi): [length, step_abs_sum,
    bend_sum]}, n_flat, n_small, target {f: (g, reason)}, end, links"""
    h, w = len(bmap), len(bmap[0])
    P = [[max(R[y][x], 0) for x in range(w)] for y in range(h)]
    facet = [[-1] * w for _ in range(h)]
    pixels, plane, building = [], [], []
    for y in range(h):
        for x in range(w):
            if bmap[y][x] < 0 or facet[y][x] >= 0:
                continue
            f = len(pixels)
            facet[y][x] = f
            stack, n = [(x, y)], 0
            while stack:
                a, b = stack.pop()
                n += 1
                for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                    u, v = a + dx, b + dy
                    if 0 <= u < w and 0 <= v < h and facet[v][u] < 0 and bmap[v][u] == bmap[y][x] and P[v][u] == P[y][x]:
                        facet[v][u] = f
                        stack.append((u, v))
            pixels.append(n)
            plane.append(P[y][x])
            building.append(bmap[y][x])
    edges = {}
    for y in range(h):
        for x in range(w):
            if bmap[y][x] < 0:
                continue
            for d in (0, 1):
                u, v = (x + 1, y) if d == 0 else (x, y + 1)
                if u >= w or v >= h or bmap[v][u] != bmap[y][x] or facet[v][u] == facet[y][x]:
                    continue
                A, B = [int(t) for t in top[y][x]], [int(t) for t in top[v][u]]
                if d == 0:
                    a_s, a_e, b_s, b_e = A[1], A[3], B[0], B[2]
                    bend = ((A[1] + A[3]) - (A[0] + A[2])) - ((B[1] + B[3]) - (B[0] + B[2]))
                else:
                    a_s, a_e, b_s, b_e = A[2], A[3], B[0], B[1]
                    bend = ((A[2] + A[3]) - (A[0] + A[1])) - ((B[2] + B[3]) - (B[0] + B[1]))
                key = (min(facet[y][x], facet[v][u]), max(facet[y][x], facet[v][u]))
                e = edges.setdefault(key, [0, 0, 0])
                e[0] += 1
                e[1] += abs(a_s - b_s) + abs(a_e - b_e)
                e[2] += bend

    def is_flat(e):
        return not e[1] > 2 * step_tol * e[0] and not e[2] > bend_tol * e[0] and not e[2] < -bend_tol * e[0]

    def outranks(g, f):
        return pixels[g] > pixels[f] or (pixels[g] == pixels[f] and g < f)

    target = {}
    for (lo, hi), e in edges.items():
        for f, g in ((lo, hi), (hi, lo)):
            by_flat = bool(merge_flat) and is_flat(e)
            if not (plane[g] > 0 and outranks(g, f) and (pixels[f] < min_pixels or by_flat)):
                continue
            if f in target:
                t = target[f]
                if not (e[0] > t[2] or (e[0] == t[2] and outranks(g, t[0]))):
                    continue
            target[f] = (g, by_flat, e[0])
    end, links = [], []
    for f in range(len(pixels)):
        g, n = f, 0
        while g in target:
            g = target[g][0]
            n += 1
        end.append(g)
        links.append(n)
    return dict(facet=facet, pixels=pixels, plane=plane, building=building, edges=edges,
                n_flat=sum(is_flat(e) for e in edges.values()), n_small=sum(p < min_pixels for p in pixels), target=target,
                end=end, links=links)


def generalise(bmap, roof, n_buildings, normal, center, z_min, z_max, bin, base_z, flat, min_pixels=0, merge_flat=False,
               step_tol=200, bend_tol=0, max_rounds=64):
    bm = np.asarray(bmap).tolist()
    R = np.asarray(roof).tolist()
    R0 = [row[:] for row in R]
    h, w = len(bm), len(bm[0])
    n_planes = len(np.asarray(z_min).reshape(-1))
    evals, tops = [], []
    rounds, converged = 0, 0
    r = 1
    while True:
        top = sr.tops(np.asarray(bm), np.asarray(R), normal, center, z_min, z_max, bin, base_z, flat)
        tops.append(top)
        ev = evaluate(bm, R, top.tolist(), min_pixels, merge_flat, step_tol, bend_tol)
        evals.append(ev)
        if not ev["target"]:
            converged = 1
            break
        if r > max_rounds:
            break
        for y in range(h):
            for x in range(w):
                f = ev["facet"][y][x]
                if f >= 0 and f in ev["target"]:
                    R[y][x] = ev["plane"][ev["end"][f]]
        rounds = r
        r += 1
    out = SimpleNamespace(roof=np.asarray(R, np.int32).reshape(h, w), rounds=rounds, converged=converged)
    first, last = evals[0], evals[-1]
    for tag, ev in (("in", first), ("out", last)):
        setattr(out, "n_facets_" + tag, len(ev["pixels"]))
        setattr(out, "n_edges_" + tag, len(ev["edges"]))
        setattr(out, "n_flat_" + tag, ev["n_flat"])
        setattr(out, "n_small_" + tag, ev["n_small"])
        fac = [0] * n_buildings
        for c in ev["building"]:
            fac[c] += 1
        setattr(out, "building_facets_" + tag, np.asarray(fac, np.int64).reshape(n_buildings))
    out.eval_facets = np.asarray([len(e["pixels"]) for e in evals], np.int64)
    out.eval_movers = np.asarray([len(e["target"]) for e in evals], np.int64)
    out.eval_movers_flat = np.asarray([sum(t[1] for t in e["target"].values()) for e in evals], np.int64)
    out.eval_movers_small = out.eval_movers - out.eval_movers_flat
    out.eval_longest_chain = np.asarray([max(e["links"], default=0) for e in evals], np.int64)
    pin, pout = [0] * (n_planes + 1), [0] * (n_planes + 1)
    chg, dsum, dmax = [0] * n_buildings, [0] * n_buildings, [0] * n_buildings
    roofed = 0
    T0, T1 = tops[0].astype(np.int64).tolist(), tops[-1].astype(np.int64).tolist()
    for y in range(h):
        for x in range(w):
            c = bm[y][x]
            if c < 0:
                continue
            p0, p1 = max(R0[y][x], 0), max(R[y][x], 0)
            pin[p0] += 1
            pout[p1] += 1
            chg[c] += R0[y][x] != R[y][x]
            roofed += p0 == 0 and p1 > 0
            d = [abs(a - b) for a, b in zip(T0[y][x], T1[y][x])]
            dsum[c] += sum(d)
            dmax[c] = max(dmax[c], max(d))
    out.plane_pixels_in, out.plane_pixels_out = np.asarray(pin, np.int64), np.asarray(pout, np.int64)
    out.building_pixels_changed = np.asarray(chg, np.int64).reshape(n_buildings)
    out.building_sum_abs_dtop = np.asarray(dsum, np.int64).reshape(n_buildings)
    out.building_max_abs_dtop = np.asarray(dmax, np.int64).reshape(n_buildings)
    out.pixels_changed, out.pixels_roofed = sum(chg), roofed
    return out
