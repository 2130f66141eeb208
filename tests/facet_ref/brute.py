"""The roof facets and their edges (include/bs_api.h, "roof facets") pixel by pixel in plain Python: a flood fill, then loops
over the pixel edges.  Also the kinds of bs_roof_edge_kinds and the text of bs_roof_edges_write_obj.  Slow on purpose:
tests/facet_ref/facet_ref.py is the vectorised restatement that must equal it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
KIND_NAMES = ("flat", "ridge", "valley", "step")
FACET_FIELDS = (("building", np.int32), ("plane", np.int32), ("start_xy", np.int32), ("pixels", np.int64), ("bbox", np.int32),
                ("inner_edges", np.int64), ("outer_edges", np.int64), ("top_min", np.int32), ("top_max", np.int32),
                ("top_sum", np.int64))
EDGE_FIELDS = (("facet", np.int32), ("building", np.int32), ("length", np.int64), ("n_dir0", np.int64), ("n_step", np.int64),
               ("step_abs_sum", np.int64), ("step_abs_max", np.int64), ("rise_sum", np.int64), ("bend_sum", np.int64),
               ("z_min", np.int32), ("z_max", np.int32), ("bbox", np.int32))
TOTALS = ("n_facets", "n_edges", "n_pixels", "n_border")
WIDTH = {"start_xy": 2, "bbox": 4, "facet": 2}  # columns of the two-dimensional arrays


def border_heights(top, x, y, d):
    """(a_s, a_e, b_s, b_e, s_A, s_B, s, e) of the pixel edge of A = (x, y) in direction d; tops as Python ints"""
    A = [int(v) for v in top[y][x]]
    if d == 0:
        B = [int(v) for v in top[y][x + 1]]
        return (A[1], A[3], B[0], B[2], (A[1] + A[3]) - (A[0] + A[2]), (B[1] + B[3]) - (B[0] + B[2]), (x + 1, y), (x + 1, y + 1))
    B = [int(v) for v in top[y + 1][x]]
    return (A[2], A[3], B[0], B[1], (A[2] + A[3]) - (A[0] + A[1]), (B[2] + B[3]) - (B[0] + B[1]), (x, y + 1), (x + 1, y + 1))


def label(bmap, roof):
    """facet[y][x] by flood fill in raster order, and the (building, plane, start) of every facet"""
    h, w = len(bmap), len(bmap[0])
    plane = [[(int(roof[y][x]) if roof[y][x] > 0 else 0) for x in range(w)] for y in range(h)]
    facet = [[-1] * w for _ in range(h)]
    heads = []
    for y in range(h):
        for x in range(w):
            if bmap[y][x] < 0 or facet[y][x] >= 0:
                continue
            f = len(heads)
            heads.append((int(bmap[y][x]), plane[y][x], x, y))
            facet[y][x] = f
            stack = [(x, y)]
            while stack:
                cx, cy = stack.pop()
                for nx, ny in ((cx - 1, cy), (cx + 1, cy), (cx, cy - 1), (cx, cy + 1)):
                    if 0 <= nx < w and 0 <= ny < h and facet[ny][nx] < 0 and bmap[ny][nx] == bmap[y][x] \
                            and plane[ny][nx] == plane[y][x]:
                        facet[ny][nx] = f
                        stack.append((nx, ny))
    return facet, heads


def pack(facet, fig, edges):
    """the result as arrays: fig is a list of dicts per facet, edges a list of dicts in ascending (lo, hi)"""
    out = SimpleNamespace(facet=np.asarray(facet, np.int32))
    for name, dt in FACET_FIELDS:
        a = np.array([f[name] for f in fig], dt)
        setattr(out, "facet_" + name, a.reshape(len(fig), WIDTH[name]) if name in WIDTH else a.reshape(len(fig)))
    for name, dt in EDGE_FIELDS:
        a = np.array([e[name] for e in edges], dt)
        setattr(out, "edge_" + name, a.reshape(len(edges), WIDTH[name]) if name in WIDTH else a.reshape(len(edges)))
    out.n_facets, out.n_edges = len(fig), len(edges)
    out.n_pixels = int(sum(f["pixels"] for f in fig))
    out.n_border = int(sum(e["length"] for e in edges))
    return out


def roof_facets(bmap, roof, top):
    bmap, roof, top = np.asarray(bmap).tolist(), np.asarray(roof).tolist(), np.asarray(top).tolist()
    h, w = len(bmap), len(bmap[0])
    facet, heads = label(bmap, roof)
    fig = [dict(building=b, plane=p, start_xy=[x, y], pixels=0, bbox=[I32_MAX, I32_MAX, I32_MIN, I32_MIN], inner_edges=0,
                outer_edges=0, top_min=I32_MAX, top_max=I32_MIN, top_sum=0) for b, p, x, y in heads]
    edges = {}
    for y in range(h):
        for x in range(w):
            c = bmap[y][x]
            if c < 0:
                continue
            F = fig[facet[y][x]]
            F["pixels"] += 1
            F["bbox"] = [min(F["bbox"][0], x), min(F["bbox"][1], y), max(F["bbox"][2], x), max(F["bbox"][3], y)]
            F["top_min"], F["top_max"] = min([F["top_min"]] + top[y][x]), max([F["top_max"]] + top[y][x])
            F["top_sum"] += sum(top[y][x])
            for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if not (0 <= nx < w and 0 <= ny < h) or bmap[ny][nx] != c:
                    F["outer_edges"] += 1
            for d, (nx, ny) in enumerate(((x + 1, y), (x, y + 1))):
                if not (nx < w and ny < h) or bmap[ny][nx] != c or facet[ny][nx] == facet[y][x]:
                    continue
                fa, fb = facet[y][x], facet[ny][nx]
                fig[fa]["inner_edges"] += 1
                fig[fb]["inner_edges"] += 1
                a_s, a_e, b_s, b_e, s_a, s_b, s, e = border_heights(top, x, y, d)
                E = edges.setdefault((min(fa, fb), max(fa, fb)), dict(
                    facet=[min(fa, fb), max(fa, fb)], building=c, length=0, n_dir0=0, n_step=0, step_abs_sum=0, step_abs_max=0,
                    rise_sum=0, bend_sum=0, z_min=I32_MAX, z_max=I32_MIN, bbox=[I32_MAX, I32_MAX, I32_MIN, I32_MIN]))
                E["length"] += 1
                E["n_dir0"] += d == 0
                E["n_step"] += (a_s, a_e) != (b_s, b_e)
                E["step_abs_sum"] += abs(a_s - b_s) + abs(a_e - b_e)
                E["step_abs_max"] = max(E["step_abs_max"], abs(a_s - b_s), abs(a_e - b_e))
                sign = 1 if fa > fb else -1  # h is the side of facet_hi
                E["rise_sum"] += sign * ((a_s - b_s) + (a_e - b_e))
                E["bend_sum"] += s_a - s_b
                E["z_min"], E["z_max"] = min(E["z_min"], a_s, a_e, b_s, b_e), max(E["z_max"], a_s, a_e, b_s, b_e)
                E["bbox"] = [min(E["bbox"][0], s[0], e[0]), min(E["bbox"][1], s[1], e[1]), max(E["bbox"][2], s[0], e[0]),
                             max(E["bbox"][3], s[1], e[1])]
    return pack(facet, fig, [edges[k] for k in sorted(edges)])


def kinds(rf, step_tol, bend_tol):
    """bs_roof_edge_kinds: uint8 [n_edges]"""
    out = []
    for length, step, bend in zip(rf.edge_length.tolist(), rf.edge_step_abs_sum.tolist(), rf.edge_bend_sum.tolist()):
        if step > 2 * step_tol * length:
            out.append(3)
        elif bend > bend_tol * length:
            out.append(1)
        elif bend < -bend_tol * length:
            out.append(2)
        else:
            out.append(0)
    return np.array(out, np.uint8)


def obj_text(rf, bmap, top, bin, kind, origin=None):
    """the file of bs_roof_edges_write_obj as bytes"""
    o = [0, 0, 0] if origin is None else [int(v) for v in origin]
    bmap, facet, top = np.asarray(bmap).tolist(), np.asarray(rf.facet).tolist(), np.asarray(top).tolist()
    h, w = len(bmap), len(bmap[0])
    number = {tuple(p): e for e, p in enumerate(np.asarray(rf.edge_facet).reshape(-1, 2).tolist())}
    segs = [[] for _ in number]
    for y in range(h):
        for x in range(w):
            for d, (nx, ny) in enumerate(((x + 1, y), (x, y + 1))):
                if bmap[y][x] < 0 or not (nx < w and ny < h) or bmap[ny][nx] != bmap[y][x] or facet[ny][nx] == facet[y][x]:
                    continue
                a_s, a_e, b_s, b_e, _, _, s, e = border_heights(top, x, y, d)
                pair = (min(facet[y][x], facet[ny][nx]), max(facet[y][x], facet[ny][nx]))
                segs[number[pair]].append((s, max(a_s, b_s), e, max(a_e, b_e)))
    out = [f"# roof edges: {len(segs)} edges, {sum(len(s) for s in segs)} segments\n"]
    nv = 0
    for e, ss in enumerate(segs):
        out.append(f"g edge_{e}_{KIND_NAMES[int(kind[e])]}\n")
        for s, zs, en, ze in ss:
            out.append(f"v {s[0] * bin + o[0]} {s[1] * bin + o[1]} {zs + o[2]}\n")
            out.append(f"v {en[0] * bin + o[0]} {en[1] * bin + o[1]} {ze + o[2]}\n")
            out.append(f"l {nv + 1} {nv + 2}\n")
            nv += 2
    return "".join(out).encode()
