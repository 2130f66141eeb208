"""Simplified outlines by brute force (include/bs_api.h, "simplified outlines"): every ring is walked half-edge by
half-edge, cut into arcs at its junction nodes, and every arc goes through a recursive Douglas-Peucker with Python
integers, straight from the definition.  Slow and obvious; tests/simplify_ref/simplify_ref.py must equal it."""
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


ob = _load("outline_brute", os.path.join(HERE, "..", "outline_ref", "brute.py"))

FIELDS = ("n_rings", "n_nodes", "n_junction_nodes", "n_arcs", "n_svertices", "rounds", "max_arc_nodes", "s_ring_vertices",
          "s_ring_area2", "s_ring_arcs", "s_ring_offset", "sxy", "sz", "s_right", "s_flag")


def pack(rings, has_z, rounds, max_arc_nodes, n_nodes, n_junction_nodes):
    """rings in the listed order: (kept [(X, Y, Z, right, flag)], arcs)"""
    verts = [v for r in rings for v in r[0]]
    area2 = []
    for kept, _ in rings:
        a = 0
        for j, v in enumerate(kept):
            u = kept[(j + 1) % len(kept)]
            a += v[0] * u[1] - u[0] * v[1]
        area2.append(a)
    return SimpleNamespace(
        n_rings=len(rings), n_nodes=n_nodes, n_junction_nodes=n_junction_nodes, n_arcs=sum(r[1] for r in rings),
        n_svertices=len(verts), rounds=rounds, max_arc_nodes=max_arc_nodes,
        s_ring_vertices=np.array([len(r[0]) for r in rings], np.int64), s_ring_area2=np.array(area2, np.int64),
        s_ring_arcs=np.array([r[1] for r in rings], np.int64),
        s_ring_offset=np.concatenate([[0], np.cumsum([len(r[0]) for r in rings])]).astype(np.int64),
        sxy=np.array([v[:2] for v in verts], np.int32).reshape(len(verts), 2),
        sz=np.array([v[2] for v in verts], np.int32) if has_z else None,
        s_right=np.array([v[3] for v in verts], np.int32), s_flag=np.array([v[4] for v in verts], np.uint8))


def far(c2, len2, num, den):
    """farther than the tolerance, exactly"""
    return c2 * den > num * len2


def douglas_peucker(arc, num, den):
    """arc: [(X, Y, corner index)] from one end node to the other, both included.  Returns (the kept positions, the depth
    of the deepest split that kept something)."""
    keep = {0, len(arc) - 1}

    def split(i, j, forced):
        if j - i < 2:
            return 0
        (sx, sy, _), (ex, ey, _) = arc[i], arc[j]
        best = None
        for m in range(i + 1, j):
            c = (ex - sx) * (arc[m][1] - sy) - (ey - sy) * (arc[m][0] - sx)
            key = (-c * c, arc[m][2])  # the greatest c^2, ties to the lowest corner index
            if best is None or key < best[0]:
                best = (key, m)
        c2, m = -best[0][0], best[1]
        if not (c2 > 0 if forced else far(c2, (ex - sx) ** 2 + (ey - sy) ** 2, num, den)):
            return 0
        keep.add(m)
        return 1 + max(split(i, m, False), split(m, j, False))

    if arc[0][2] != arc[-1][2]:
        depth = split(0, len(arc) - 1, True)  # (the first split of every arc is forced)
    else:  # a closed arc: the farthest node from the start, then a forced first split of both parts
        sx, sy, _ = arc[0]
        f = min(range(1, len(arc) - 1), key=lambda m: (-((arc[m][0] - sx) ** 2 + (arc[m][1] - sy) ** 2), arc[m][2]))
        keep.add(f)
        depth = max(split(0, f, True), split(f, len(arc) - 1, True))
    return keep, depth


def ring_nodes(label, top, h0):
    """the nodes of the ring that starts at half-edge h0, in walk order: (X, Y, Z, right, junction, corner index)"""
    h, w = label.shape

    def lab(x, y):
        return max(int(label[y, x]), -1) if 0 <= x < w and 0 <= y < h else -1

    def inside(r, p):
        return 0 <= r[0] < w and 0 <= r[1] < h and label[r[1], r[0]] == label[p[1], p[0]]

    def step(p, k):
        return (p[0] + ob.DELTA[k][0], p[1] + ob.DELTA[k][1])

    def succ(p, k):
        p1 = step(p, (k + 1) % 4)
        q = step(p1, k)
        if not inside(p1, p):
            return p, (k + 1) % 4
        if not inside(q, p):
            return p1, k
        return q, (k + 3) % 4

    start = ((h0 // 4 % w, h0 // 4 // w), h0 % 4)
    walk, cur = [], start
    while not walk or cur != start:
        walk.append(cur)
        cur = succ(*cur)
    nodes = []
    for j, (p, k) in enumerate(walk):
        X, Y = p[0] + ob.START[k][0], p[1] + ob.START[k][1]
        a, b, c, d = lab(X - 1, Y - 1), lab(X, Y - 1), lab(X - 1, Y), lab(X, Y)
        junction = len({a, b, c, d}) >= 3 or (a == d and b == c and a != b)
        if walk[j - 1][1] != k or junction:
            z = int(top[p[1]][p[0]][ob.ZIDX[k]]) if top is not None else 0
            nodes.append((X, Y, z, lab(*step(p, k)), junction, Y * (w + 1) + X))
    return nodes


def simplify(label, top=None, n_labels=None, num=0, den=1):
    label = np.asarray(label, np.int64)
    plain = ob.outlines(label, top, n_labels)
    rings, rounds, max_arc, n_nodes, n_junction = [], 0, 0, 0, 0
    for r in range(plain.n_rings):
        nodes = ring_nodes(label, top, int(plain.ring_start[r]))
        nn = len(nodes)
        junc = [j for j in range(nn) if nodes[j][4]]
        n_nodes += nn
        n_junction += len(junc)
        starts = junc if junc else [min(range(nn), key=lambda j: nodes[j][5])]
        kept = set()
        for a, s in enumerate(starts):
            e = starts[(a + 1) % len(starts)]
            count = (e - s - 1) % nn + 2  # the nodes of the arc, both ends included (a whole ring: its start twice)
            arc = [nodes[(s + m) % nn] for m in range(count)]
            max_arc = max(max_arc, count)
            keep, depth = douglas_peucker([(v[0], v[1], v[5]) for v in arc], num, den)
            rounds = max(rounds, depth)
            kept |= {(s + m) % nn for m in keep}
        out = [(nodes[j][0], nodes[j][1], nodes[j][2], nodes[j][3], int(nodes[j][4]) | (0 if junc else 2 * (j == starts[0])))
               for j in sorted(kept)]
        rings.append((out, len(starts)))
    return plain, pack(rings, top is not None, rounds, max_arc, n_nodes, n_junction)


def obj_text(plain, s, bin, num, den, origin=None):
    """the OBJ of bs_simple_outlines_write_obj as bytes"""
    org = (0, 0, 0) if origin is None else tuple(int(v) for v in origin)
    lines = [f"# simplified outlines: {plain.n_labels} labels, {s.n_rings} rings, {s.n_svertices} vertices, tol2 {num}/{den}"]
    for r in range(s.n_rings):
        lab = int(plain.ring_label[r])
        kind = "outer" if plain.ring_area2[r] > 0 else "hole"
        lines.append(f"g label_{lab}_ring_{r - int(plain.label_ring_offset[lab])}_{kind}")
        a, b = int(s.s_ring_offset[r]), int(s.s_ring_offset[r + 1])
        for v in range(a, b):
            z = int(s.sz[v]) if s.sz is not None else 0
            lines.append(f"v {int(s.sxy[v, 0]) * bin + org[0]} {int(s.sxy[v, 1]) * bin + org[1]} {z + org[2]}")
        lines.append("l " + " ".join(str(v + 1) for v in list(range(a, b)) + [a]))
    return ("\n".join(lines) + "\n").encode()
