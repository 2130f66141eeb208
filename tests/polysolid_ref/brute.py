"""Polygon solids by brute force (include/bs_api.h, "polygon solids"): the definition taken literally with Python integers,
dicts and lists on the objects of tests/triangulate_ref and tests/uncross_ref (imported, not modified): the vertices as a
sorted set of quadruples, the twin of a segment looked up by its corners and label, the vertices of a column found by walking
its sorted heights.  Slow and obvious; tests/polysolid_ref/polysolid_ref.py must equal it."""
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


tref = _load("triangulate_ref", os.path.join(HERE, "..", "triangulate_ref", "triangulate_ref.py"))
tbrute, uref = tref.brute, tref.uref

MESH = ("vertex", "face_offset", "face_index", "face_building", "face_kind")
FIGURES = ("status", "labels", "vertices", "faces", "roof_faces", "wall_faces", "crossing_walls", "max_wall_vertices", "z_min",
           "z_max", "area2", "volume6")
TOTALS = ("n_open_buildings", "n_vertices", "n_faces", "n_indices", "n_roof_faces", "n_wall_faces", "n_crossing_walls",
          "max_wall_vertices_all", "total_area2", "total_volume6")
FIELDS = MESH + FIGURES + TOTALS
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
Z_LIMIT = 1 << 24


def orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def pack(nb, vertex, faces, fig):
    """vertex: [(X * bin, Y * bin, Z, c)], faces: [(building, kind, [vertex numbers])], fig: name -> list per building"""
    sizes = [len(f[2]) for f in faces]
    out = SimpleNamespace(
        n_buildings=nb, vertex=np.array(vertex, np.int32).reshape(len(vertex), 4),
        face_offset=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32),
        face_index=np.array([v for f in faces for v in f[2]], np.int32), face_building=np.array([f[0] for f in faces], np.int32),
        face_kind=np.array([f[1] for f in faces], np.uint8))
    for k in FIGURES:
        setattr(out, k, np.array(fig[k], np.int32 if k in ("status", "z_min", "z_max") else np.int64).reshape(nb))
    out.n_open_buildings = int(sum(fig["status"]))
    out.n_vertices, out.n_faces, out.n_indices = len(vertex), len(faces), int(sum(sizes))
    out.n_roof_faces, out.n_wall_faces = int(sum(fig["roof_faces"])), int(sum(fig["wall_faces"]))
    out.n_crossing_walls = int(sum(fig["crossing_walls"]))
    out.max_wall_vertices_all = int(max(fig["max_wall_vertices"], default=0))
    out.total_area2, out.total_volume6 = int(sum(fig["area2"])), int(sum(fig["volume6"]))
    return out


def poly_solids(plain, clean, tri, label_building, n_buildings, bin, base_z):
    """the polygon solids over the triangles `tri` of the clean outlines `clean` (with sz) over the plain outlines `plain`"""
    nl, nb = int(tri.n_labels), int(n_buildings)
    lb = [int(v) for v in label_building]
    assert len(lb) == nl and all(0 <= v < nb for v in lb)
    P = [tuple(p) for p in np.asarray(clean.sxy, np.int64).reshape(-1, 2).tolist()]
    Z = [int(v) for v in np.asarray(clean.sz).tolist()] if len(P) else []
    right = [int(v) for v in np.asarray(clean.s_right).tolist()]
    soff = [int(v) for v in clean.s_ring_offset]
    lro = [int(v) for v in plain.label_ring_offset]
    status = [int(v) for v in tri.label_status]
    assert all(abs(z - base_z) < Z_LIMIT for z in Z)
    is_open = [0] * nb
    for l in range(nl):
        if status[l] in (tbrute.NO_BRIDGE, tbrute.STALLED):
            is_open[lb[l]] = 1
    rings = {l: [(soff[r], soff[r + 1]) for r in range(lro[l], lro[l + 1])] for l in range(nl)}
    nxt, label_of = {}, {}
    for l in range(nl):
        for a, b in rings[l]:
            for i in range(a, b):
                nxt[i], label_of[i] = (i + 1 if i + 1 < b else a), l
    # the vertices: one per distinct quadruple, by (c, Y, X, Z)
    quads = set()
    for i, l in label_of.items():
        c = lb[l]
        if not is_open[c]:
            quads |= {(c, P[i][1], P[i][0], Z[i]), (c, P[i][1], P[i][0], base_z)}
    order = sorted(quads)
    number = {q: n for n, q in enumerate(order)}
    vertex = [(x * bin, y * bin, z, c) for c, y, x, z in order]
    column = {}
    for c, y, x, z in order:
        column.setdefault((c, x, y), []).append(z)
    segment = {(P[i], P[nxt[i]], l): i for i, l in label_of.items()}

    def num(c, i, z):
        return number[(c, P[i][1], P[i][0], z)]

    def between(c, i, z_from, z_to):
        """the vertices of the column of (c, i) strictly between two heights, walking from z_from"""
        zs = [z for z in column[(c, P[i][0], P[i][1])] if min(z_from, z_to) < z < max(z_from, z_to)]
        return [num(c, i, z) for z in (zs if z_from < z_to else zs[::-1])]

    fig = {k: [0] * nb for k in FIGURES}
    fig["status"] = is_open
    fig["z_min"], fig["z_max"] = [INT32_MAX] * nb, [INT32_MIN] * nb
    for l in range(nl):
        fig["labels"][lb[l]] += 1
    for c, y, x, z in order:
        fig["vertices"][c] += 1
    faces = []
    for l in range(nl):
        c = lb[l]
        if is_open[c] or status[l] != tbrute.OK:
            continue
        tris = np.asarray(tri.tri)[int(tri.tri_offset[l]):int(tri.tri_offset[l + 1])].tolist()
        for a, b, d in tris:
            faces.append((c, 0, [num(c, a, Z[a]), num(c, b, Z[b]), num(c, d, Z[d])]))
            o = orient(P[a], P[b], P[d])
            fig["roof_faces"][c] += 1
            fig["area2"][c] += o
            fig["volume6"][c] += o * (Z[a] + Z[b] + Z[d] - 3 * base_z)
        for a, b, d in tris:
            faces.append((c, 1, [num(c, d, base_z), num(c, b, base_z), num(c, a, base_z)]))
        for ra, rb in rings[l]:
            for s in range(ra, rb):
                e, R = nxt[s], right[s]
                a_s, a_e = Z[s], Z[e]
                fig["z_min"][c], fig["z_max"][c] = min(fig["z_min"][c], a_s), max(fig["z_max"][c], a_s)
                emits = True
                if R >= 0 and lb[R] == c:
                    t = segment.get((P[e], P[s], R))
                    if t is None or right[t] != l:
                        raise AssertionError("a twin is missing or has the wrong labels")
                    b_e, b_s = Z[t], Z[nxt[t]]
                    emits = l < R
                else:
                    b_s = b_e = base_z
                if (a_s, a_e) == (b_s, b_e) or not emits:
                    continue
                poly = [num(c, e, a_e), num(c, s, a_s)] + between(c, s, a_s, b_s)
                if b_s != a_s:
                    poly.append(num(c, s, b_s))
                if b_e != a_e:
                    poly.append(num(c, e, b_e))
                poly += between(c, e, b_e, a_e)
                faces.append((c, 2, poly))
                fig["wall_faces"][c] += 1
                fig["crossing_walls"][c] += (a_s - b_s) * (a_e - b_e) < 0
                fig["max_wall_vertices"][c] = max(fig["max_wall_vertices"][c], len(poly))
    for f in faces:
        fig["faces"][f[0]] += 1
    return pack(nb, vertex, faces, fig)


def same(a, b, fields=FIELDS):
    """None if the two results are equal, else the name of the first field that differs"""
    return tbrute.same(a, b, fields)


def obj_text(s, origin=None):
    """the OBJ of bs_solids_write_obj for this mesh as bytes"""
    org = origin if origin is not None else (0, 0, 0)
    fb = np.asarray(s.face_building).tolist()
    used = sorted(set(fb))
    out = [f"# solids: {len(used)} buildings, {len(s.vertex)} vertices, {len(fb)} faces\n"]
    for x, y, z, _ in np.asarray(s.vertex).tolist():
        out.append(f"v {x + org[0]} {y + org[1]} {z + org[2]}\n")
    off, idx = np.asarray(s.face_offset).tolist(), np.asarray(s.face_index).tolist()
    for c in used:
        out.append(f"o building_{c}\n")
        for f, b in enumerate(fb):
            if b == c:
                out.append("f " + " ".join(str(v + 1) for v in idx[off[f]:off[f + 1]]) + "\n")
    return "".join(out).encode()
