"""Outline triangles by brute force (include/bs_api.h, "outline triangles"), the definition taken literally with Python
integers and lists, on the rings of tests/uncross_ref (imported, not modified): per label the bridges in the order of the
holes -- every occurrence of every list a candidate, every ring segment and every earlier bridge a blocker -- then the ear
scan list by list.  Slow and obvious; tests/triangulate_ref/triangulate_ref.py must equal it."""
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


uref = _load("uncross_ref", os.path.join(HERE, "..", "uncross_ref", "uncross_ref.py"))

OK, NO_BRIDGE, STALLED, EMPTY = 0, 1, 2, 3
ARRAYS = ("tri", "tri_offset", "bridge", "label_status", "label_area2", "label_tests")
TOTALS = ("n_triangles", "n_failed_labels", "n_bridges", "n_tests", "max_label_occurrences")
FIELDS = ARRAYS + TOTALS  # what the brute force and the restatement share


def orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def cross(u, v):
    return u[0] * v[1] - u[1] * v[0]


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1])


def in_cone(p, v, n, d):
    """the direction d in the cone at v between its predecessor p and its successor n"""
    if orient(p, v, n) > 0:
        return cross(sub(n, v), d) > 0 and cross(d, sub(p, v)) > 0
    return not (cross(sub(p, v), d) >= 0 and cross(d, sub(n, v)) >= 0)


def on_closed(a, b, p):
    return orient(a, b, p) == 0 and min(a[0], b[0]) <= p[0] <= max(a[0], b[0]) and min(a[1], b[1]) <= p[1] <= max(a[1], b[1])


def blocks(s, e, M, V):
    """the segment s-e blocks M-V"""
    o1, o2, o3, o4 = orient(M, V, s), orient(M, V, e), orient(s, e, M), orient(s, e, V)
    if o1 * o2 < 0 and o3 * o4 < 0:
        return True
    if any(p != M and p != V and on_closed(M, V, p) for p in (s, e)):
        return True
    return any(on_closed(s, e, p) and p != s and p != e for p in (M, V))


def triangulate_label(P, rings):
    """P: the position of every vertex; rings: (ring, its vertices in order, outer) in ring order.  Returns (status,
    triangles, {hole ring: (M, V)}, tests)."""
    vert, nxt, prv = [], [], []  # occurrences

    def add_ring(vs):
        base = len(vert)
        for i, v in enumerate(vs):
            vert.append(v)
            nxt.append(base + (i + 1) % len(vs))
            prv.append(base + (i - 1) % len(vs))
        return base

    segments = [(P[vs[i]], P[vs[(i + 1) % len(vs)]]) for _, vs, _ in rings for i in range(len(vs))]
    firsts = [add_ring(vs) for _, vs, outer in rings if outer]
    in_list = set(range(len(vert)))
    holes = sorted((min((P[v][0], P[v][1], v) for v in vs), r, vs) for r, vs, outer in rings if not outer)
    bridges, done = {}, []
    for (_, _, M), r, vs in holes:
        base = add_ring(vs)
        m = base + vs.index(M)
        valid = []
        for o in sorted(in_list):
            V = vert[o]
            if P[V] == P[M]:
                continue
            if not in_cone(P[vert[prv[o]]], P[V], P[vert[nxt[o]]], sub(P[M], P[V])):
                continue
            if not in_cone(P[vert[prv[m]]], P[M], P[vert[nxt[m]]], sub(P[V], P[M])):
                continue
            if any(blocks(s, e, P[M], P[V]) for s, e in segments) or any(blocks(s, e, P[M], P[V]) for s, e in done):
                continue
            valid.append(((P[V][0] - P[M][0]) ** 2 + (P[V][1] - P[M][1]) ** 2, V, o))
        if not valid:
            return NO_BRIDGE, [], {}, 0
        assert len({v for _, v, _ in valid}) == len(valid), "two valid occurrences of one vertex"
        _, V, o = min(valid)
        # ... V, M, (the hole from M round), M', V', ...
        m2, v2 = len(vert), len(vert) + 1
        vert.extend([M, V])
        nxt.extend([v2, nxt[o]])
        prv.extend([prv[m], m2])
        prv[nxt[o]] = v2
        nxt[prv[m]] = m2
        nxt[o], prv[m] = m, o
        in_list |= set(range(base, base + len(vs))) | {m2, v2}
        bridges[r] = (M, V)
        done.append((P[M], P[V]))
    tris, tests = [], 0
    for first in firsts:
        left, o = 1, nxt[first]
        while o != first:
            left, o = left + 1, nxt[o]
        stop = cur = first
        while left > 3:
            b, a, c = cur, prv[cur], nxt[cur]
            A, B, C = P[vert[a]], P[vert[b]], P[vert[c]]
            tests += 1
            ear = orient(A, B, C) > 0
            if ear:
                q = nxt[c]
                while q != a and ear:
                    Q = P[vert[q]]
                    if Q != A and Q != B and Q != C and orient(A, B, Q) >= 0 and orient(B, C, Q) >= 0 and orient(C, A, Q) >= 0:
                        ear = False
                    q = nxt[q]
            if ear:
                tris.append((vert[a], vert[b], vert[c]))
                nxt[a], prv[c] = c, a
                left -= 1
                cur = stop = nxt[c]
            else:
                cur = nxt[cur]
                if cur == stop:
                    return STALLED, [], {}, tests
        tris.append((vert[prv[cur]], vert[cur], vert[nxt[cur]]))
    return OK, tris, bridges, tests


def triangulate(plain, clean):
    """the outline triangles of the clean outlines `clean` over the plain outlines `plain` (of uncross_ref.clean)"""
    nl, nr = int(plain.n_labels), int(clean.n_rings)
    P = [(int(x), int(y)) for x, y in np.asarray(clean.sxy).reshape(-1, 2).tolist()]
    lro = [int(v) for v in plain.label_ring_offset]
    soff = [int(v) for v in clean.s_ring_offset]
    tri, tri_offset, status, area2, tests = [], [0], [], [], []
    bridge = [[-1, -1] for _ in range(nr)]
    max_occ = 0
    for l in range(nl):
        rings = [(r, list(range(soff[r], soff[r + 1])), int(plain.ring_area2[r]) > 0) for r in range(lro[l], lro[l + 1])]
        if not rings:
            status.append(EMPTY)
            area2.append(0)
            tests.append(0)
            tri_offset.append(len(tri))
            continue
        nv, nh = sum(len(vs) for _, vs, _ in rings), sum(not o for _, _, o in rings)
        n = nv + 2 * nh - 2 * (len(rings) - nh)
        max_occ = max(max_occ, nv + 2 * nh)
        st, t, br, nt = triangulate_label(P, rings)
        if st == OK:
            assert len(t) == n, (l, len(t), n)
            for r, mv in br.items():
                bridge[r] = list(mv)
        else:
            t = [(-1, -1, -1)] * n
        status.append(st)
        area2.append(sum(orient(P[a], P[b], P[c]) for a, b, c in t) if st == OK else 0)
        tests.append(nt)
        tri.extend(t)
        tri_offset.append(len(tri))
    return SimpleNamespace(
        n_labels=nl, tri=np.array(tri, np.int32).reshape(-1, 3), tri_offset=np.array(tri_offset, np.int64),
        bridge=np.array(bridge, np.int32).reshape(-1, 2), label_status=np.array(status, np.int32),
        label_area2=np.array(area2, np.int64), label_tests=np.array(tests, np.int64), n_triangles=len(tri),
        n_failed_labels=sum(s in (NO_BRIDGE, STALLED) for s in status), n_bridges=sum(b[0] >= 0 for b in bridge),
        n_tests=sum(tests), max_label_occurrences=max_occ)


def same(a, b, fields=FIELDS):
    """None if the two results are equal, else the name of the first field that differs"""
    for f in fields:
        u, v = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        if u.shape != v.shape or not np.array_equal(u.astype(np.int64), v.astype(np.int64)):
            return f
    return None


def obj_text(t, clean, bin, origin=None):
    """the OBJ of bs_outline_triangles_write_obj as bytes"""
    org = origin if origin is not None else (0, 0, 0)
    out = [f"# outline triangles: {t.n_labels} labels, {len(clean.sxy)} vertices, {t.n_triangles} triangles, "
           f"{t.n_failed_labels} failed labels, {t.n_bridges} bridges\n"]
    z = clean.sz if clean.sz is not None else np.zeros(len(clean.sxy), np.int64)
    for (x, y), zz in zip(np.asarray(clean.sxy).tolist(), np.asarray(z).tolist()):
        out.append(f"v {x * bin + org[0]} {y * bin + org[1]} {zz + org[2]}\n")
    for l in range(t.n_labels):
        if t.label_status[l] != OK:
            continue
        out.append(f"g label_{l}\n")
        for a, b, c in t.tri[int(t.tri_offset[l]):int(t.tri_offset[l + 1])].tolist():
            out.append(f"f {a + 1} {b + 1} {c + 1}\n")
    return "".join(out).encode()
