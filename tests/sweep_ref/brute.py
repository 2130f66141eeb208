"""Clean outlines with sweeps by brute force (include/bs_api.h, "clean outlines", paragraph "Sweeps"), the definition taken
literally with Python integers: `clean` of tests/uncross_ref/brute.py restated (that file is imported, not modified) with, in
every detection, EVERY kept vertex position against EVERY lens -- the boundary test, then the winding number by the signed
crossings of the ray from w in +X, half-open in Y.  Mode 0 is the existing brute force; mode 1 detects and reports; mode 2
marks conflicting and sweeping segments alike.  Slow and obvious; tests/sweep_ref/sweep_ref.py must equal it."""
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


ub = _load("uncross_brute", os.path.join(HERE, "..", "uncross_ref", "brute.py"))
sb, ob = ub.sb, ub.ob
orient, on_closed = ub.orient, ub.on_closed

F_REPAIRED, F_MARKED, F_SWEEPING = ub.F_REPAIRED, ub.F_MARKED, 16  # bits 2, 3 and 4 of s_flag
SWEEP_TOTALS = ("n_lens_segments_first", "n_sweeping_first", "n_sweeping_only_first", "n_swept_pairs_first", "max_abs_winding",
                "sweep_rounds", "n_sweeping_left")
FIELDS = ub.FIELDS  # of the clean result
ALL_FIELDS = FIELDS + SWEEP_TOTALS  # what the brute force and the restatement share


def winding(poly, w):
    """the winding number of the closed polygon (a list of points) around w, or None where w lies on its boundary"""
    n, wn = len(poly), 0
    for i in range(n):
        p, q = poly[i], poly[(i + 1) % n]
        if on_closed(p, q, w):
            return None
        o = orient(p, q, w)
        if p[1] <= w[1] < q[1] and o > 0:
            wn += 1
        elif q[1] <= w[1] < p[1] and o < 0:
            wn -= 1
    return wn


def lens_of(nodes, a, b):
    """the lens of the segment a -> b of a ring: its polygon, or None without interior nodes"""
    inner = ub.between(a, b, len(nodes))
    if not inner or a == b:
        return None
    return [nodes[a][:2]] + [nodes[m][:2] for m in inner] + [nodes[b][:2]]


def clean(label, top=None, n_labels=None, num=0, den=1, max_rounds=-1, mode=2, trace=None):
    """returns (the plain outlines, the clean outlines with the sweep figures as attributes); trace: a dict that receives,
    per detection, the swept (position, ring, left node, winding) tuples"""
    label = np.asarray(label, np.int64)
    plain = ob.outlines(label, top, n_labels)
    ring_nodes, kept, arcs, dp_rounds, max_arc, n_junction = [], [], [], 0, 0, 0
    for r in range(plain.n_rings):  # the simplified outlines, ring by ring
        nodes = sb.ring_nodes(label, top, int(plain.ring_start[r]))
        nn = len(nodes)
        junc = [j for j in range(nn) if nodes[j][4]]
        n_junction += len(junc)
        starts = junc if junc else [min(range(nn), key=lambda j: nodes[j][5])]
        keep = set()
        for a, s in enumerate(starts):
            e = starts[(a + 1) % len(starts)]
            count = (e - s - 1) % nn + 2
            arc = [nodes[(s + m) % nn] for m in range(count)]
            max_arc = max(max_arc, count)
            k, depth = sb.douglas_peucker([(v[0], v[1], v[5]) for v in arc], num, den)
            dp_rounds = max(dp_rounds, depth)
            keep |= {(s + m) % nn for m in k}
        ring_nodes.append(nodes)
        kept.append(keep)
        arcs.append((len(starts), bool(junc), starts[0]))
    before = [set(k) for k in kept]
    n_nodes = sum(len(n) for n in ring_nodes)
    rounds, n_marked_first, fig, detections = 0, None, None, []
    max_w, sweep_rounds = 0, 0
    while True:
        segs = [(r,) + s for r in range(plain.n_rings) for s in ub.ring_segments(ring_nodes[r], kept[r], int(plain.ring_label[r]))]
        marked = set()
        for i in range(len(segs)):
            for j in range(i + 1, len(segs)):
                s, t = segs[i][3], segs[j][3]
                if (max(s[0][0], s[1][0]) < min(t[0][0], t[1][0]) or max(t[0][0], t[1][0]) < min(s[0][0], s[1][0]) or
                        max(s[0][1], s[1][1]) < min(t[0][1], t[1][1]) or max(t[0][1], t[1][1]) < min(s[0][1], s[1][1])):
                    continue
                if ub.conflict_kinds(s, t):
                    marked |= {i, j}
        sweeping, pairs, n_lens = set(), [], 0
        if mode:
            positions = sorted({ring_nodes[r][j][:2] for r in range(plain.n_rings) for j in kept[r]})
            for i, (r, a, b, _) in enumerate(segs):
                poly = lens_of(ring_nodes[r], a, b)
                if poly is None:
                    continue
                n_lens += 1
                for w in positions:
                    wn = winding(poly, w)
                    if wn:
                        sweeping.add(i)
                        pairs.append((w, r, a, wn))
                        max_w = max(max_w, abs(wn))
        detections.append(pairs)
        if n_marked_first is None:
            n_marked_first = len(marked)
            fig = (n_lens, len(sweeping), len(sweeping - marked), len(pairs))
        todo = marked | sweeping if mode == 2 else marked
        if not todo or rounds == max_rounds:
            break
        if rounds >= n_nodes:
            raise RuntimeError("more repair rounds than nodes")
        if mode == 2 and sweeping:
            sweep_rounds += 1
        grew = False
        for i in sorted(todo):
            r, a, b, (p0, p1, _, _) = segs[i]
            nodes = ring_nodes[r]
            inner = ub.between(a, b, len(nodes))
            if not inner:
                continue
            c2 = {m: orient(p0, p1, nodes[m][:2]) ** 2 for m in inner}
            pick = min(inner, key=lambda m: (-c2[m], nodes[m][5]))
            assert c2[pick] > 0
            kept[r].add(pick)
            grew = True
        if not grew:
            raise RuntimeError("a repair round kept nothing")
        rounds += 1
    still = {(segs[i][0], segs[i][1]) for i in marked}
    swept = {(segs[i][0], segs[i][1]) for i in sweeping}
    rings = []
    for r in range(plain.n_rings):
        nodes = ring_nodes[r]
        n_arcs, has_junction, start = arcs[r]
        out = [(nodes[j][0], nodes[j][1], nodes[j][2], nodes[j][3],
                int(nodes[j][4]) | (0 if has_junction else 2 * (j == start)) | (F_REPAIRED if j not in before[r] else 0) |
                (F_MARKED if (r, j) in still else 0) | (F_SWEEPING if (r, j) in swept else 0)) for j in sorted(kept[r])]
        rings.append((out, n_arcs))
    res = sb.pack(rings, top is not None, dp_rounds, max_arc, n_nodes, n_junction)
    res.n_svertices_before = sum(len(k) for k in before)
    res.n_marked_first = n_marked_first
    res.n_marked_left = len(marked)
    res.n_forced = res.n_svertices - res.n_svertices_before
    res.repair_rounds = rounds
    res.mode = mode
    res.n_lens_segments_first, res.n_sweeping_first, res.n_sweeping_only_first, res.n_swept_pairs_first = fig
    res.max_abs_winding, res.sweep_rounds, res.n_sweeping_left = max_w, sweep_rounds, len(sweeping)
    if trace is not None:
        trace["detections"] = detections
    return plain, res


def first_detection(ring_xy, kept):
    """For runs too large for `clean`: the sweeping segments of one detection from the rings' node positions (a list per
    ring, in walk order) and their kept node numbers (sorted).  Every lens against every kept position inside the lens's
    box -- a position outside the box of a polygon has winding 0 -- with Python integers.  Returns (the sorted
    (ring, x, y) of the left nodes of the sweeping segments, the (position, segment) pairs, the greatest |winding|)."""
    pos = np.array(sorted({ring_xy[r][j] for r in range(len(ring_xy)) for j in kept[r]}), np.int64).reshape(-1, 2)
    left, pairs, max_w = [], 0, 0
    for r, nodes in enumerate(ring_xy):
        k = kept[r]
        for a, b in zip(k, k[1:] + k[:1]):
            poly = lens_of(nodes, a, b)
            if poly is None:
                continue
            xs, ys = [p[0] for p in poly], [p[1] for p in poly]
            box = pos[(pos[:, 0] >= min(xs)) & (pos[:, 0] <= max(xs)) & (pos[:, 1] >= min(ys)) & (pos[:, 1] <= max(ys))]
            wns = [winding(poly, (int(x), int(y))) for x, y in box]
            wns = [abs(w) for w in wns if w]
            if wns:
                left.append((r,) + tuple(nodes[a][:2]))
                pairs += len(wns)
                max_w = max(max_w, max(wns))
    return sorted(left), pairs, max_w
