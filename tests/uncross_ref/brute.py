"""Clean outlines by brute force (include/bs_api.h, "clean outlines"), the definition taken literally: the rings, nodes
and arcs of tests/simplify_ref/brute.py, its Douglas-Peucker per arc, then rounds of ALL pairs of kept segments with
Python integers -- twins apart, two segments conflict iff their closed segments have a common point that is not an end
point of both -- and every marked segment with nodes between its ends keeps its Douglas-Peucker choice, until a round
marks nothing.  Slow and obvious; tests/uncross_ref/uncross_ref.py must equal it."""
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


sb = _load("simplify_brute", os.path.join(HERE, "..", "simplify_ref", "brute.py"))
ob = sb.ob

F_REPAIRED, F_MARKED = 4, 8  # bits 2 and 3 of s_flag
TOTALS = ("n_svertices_before", "n_marked_first", "n_marked_left", "n_forced", "repair_rounds")
FIELDS = sb.FIELDS + TOTALS  # what the brute force and the restatement share
KINDS = ("cross", "touch", "overlap", "overlap_at_shared_end")


def orient(a, b, p):
    return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])


def on_closed(a, b, p):
    """p on the closed segment a-b"""
    return orient(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def conflict_kinds(s, t):
    """s, t: (P0, P1, left, right).  The kinds of conflict between the two segments: the empty set for twins and for
    segments that meet at most in a common end point of both."""
    (a0, a1, al, ar), (b0, b1, bl, br) = s, t
    if a0 == b1 and a1 == b0 and al == br and ar == bl:
        return set()
    out = set()
    d = (orient(b0, b1, a0), orient(b0, b1, a1), orient(a0, a1, b0), orient(a0, a1, b1))
    if d[0] * d[1] < 0 and d[2] * d[3] < 0:
        out.add("cross")
    if d == (0, 0, 0, 0):  # collinear: more than a point in common?
        lo, hi = max(min(a0, a1), min(b0, b1)), min(max(a0, a1), max(b0, b1))
        if lo < hi:
            out.add("overlap")
            if {a0, a1} & {b0, b1}:
                out.add("overlap_at_shared_end")
    else:
        ends = [(p, b0, b1) for p in (a0, a1)] + [(p, a0, a1) for p in (b0, b1)]
        if any(on_closed(u, v, p) and p != u and p != v for p, u, v in ends):
            out.add("touch")
    return out


def ring_segments(nodes, kept, label):
    """the segments of one ring: (position of the left kept node, of the right one, (P0, P1, left, right))"""
    k = sorted(kept)
    return [(a, b, ((nodes[a][0], nodes[a][1]), (nodes[b][0], nodes[b][1]), label, nodes[a][3]))
            for a, b in zip(k, k[1:] + k[:1])]


def between(a, b, nn):
    """the node positions strictly between a and b in walk order"""
    out, m = [], (a + 1) % nn
    while m != b:
        out.append(m)
        m = (m + 1) % nn
    return out


def clean(label, top=None, n_labels=None, num=0, den=1, max_rounds=-1, trace=None):
    """returns (the plain outlines, the clean outlines); trace: a dict that receives the kinds of conflict met, the marked
    segments without interior nodes and whether a twin pair met"""
    label = np.asarray(label, np.int64)
    plain = ob.outlines(label, top, n_labels)
    stats = dict({k: 0 for k in KINDS}, marked_without_interior=0, twin_pairs=0)
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
    rounds, n_marked_first = 0, None
    while True:
        segs = [(r,) + s for r in range(plain.n_rings) for s in ring_segments(ring_nodes[r], kept[r], int(plain.ring_label[r]))]
        marked = set()
        for i in range(len(segs)):
            for j in range(i + 1, len(segs)):
                s, t = segs[i][3], segs[j][3]
                if (max(s[0][0], s[1][0]) < min(t[0][0], t[1][0]) or max(t[0][0], t[1][0]) < min(s[0][0], s[1][0]) or
                        max(s[0][1], s[1][1]) < min(t[0][1], t[1][1]) or max(t[0][1], t[1][1]) < min(s[0][1], s[1][1])):
                    continue  # (closed segments whose boxes are apart have no common point)
                if s[0] == t[1] and s[1] == t[0] and s[2] == t[3] and s[3] == t[2]:
                    stats["twin_pairs"] += 1
                kinds = conflict_kinds(s, t)
                if kinds:
                    marked |= {i, j}
                    for k in kinds:
                        stats[k] += 1
        if n_marked_first is None:
            n_marked_first = len(marked)
        if not marked or rounds == max_rounds:
            break
        if rounds >= n_nodes:
            raise RuntimeError("more repair rounds than nodes")
        grew = False
        for i in sorted(marked):
            r, a, b, (p0, p1, _, _) = segs[i]
            nodes = ring_nodes[r]
            inner = between(a, b, len(nodes))
            if not inner:
                stats["marked_without_interior"] += 1
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
    rings = []
    for r in range(plain.n_rings):
        nodes = ring_nodes[r]
        n_arcs, has_junction, start = arcs[r]
        out = [(nodes[j][0], nodes[j][1], nodes[j][2], nodes[j][3],
                int(nodes[j][4]) | (0 if has_junction else 2 * (j == start)) | (F_REPAIRED if j not in before[r] else 0) |
                (F_MARKED if (r, j) in still else 0)) for j in sorted(kept[r])]
        rings.append((out, n_arcs))
    res = sb.pack(rings, top is not None, dp_rounds, max_arc, n_nodes, n_junction)
    res.n_svertices_before = sum(len(k) for k in before)
    res.n_marked_first = n_marked_first
    res.n_marked_left = len(marked)
    res.n_forced = res.n_svertices - res.n_svertices_before
    res.repair_rounds = rounds
    if trace is not None:
        trace.update(stats)
    return plain, res


def obj_text(plain, s, bin, num, den, origin=None):
    """the OBJ of bs_clean_outlines_write_obj as bytes: the simplified writer's with a first line of its own"""
    body = sb.obj_text(plain, s, bin, num, den, origin).split(b"\n", 1)[1]
    head = (f"# clean outlines: {plain.n_labels} labels, {s.n_rings} rings, {s.n_svertices} vertices, tol2 {num}/{den}, "
            f"repair_rounds {s.repair_rounds}, n_forced {s.n_forced}\n")
    return head.encode() + body
