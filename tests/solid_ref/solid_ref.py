"""numpy restatement of the solids (include/bs_api.h, "solids"): tops, vertices, faces and figures, vectorised over the
image so that a million pixels take seconds.  tests/solid_ref/brute.py is the per-pixel form it must equal.  The height
function is tests/roof_ref/roof_ref.py's: the one f64 division apart everything is an exact integer."""
from __future__ import annotations

import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "roof_ref"))
import roof_ref as rr  # noqa: E402

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
NO_KEY = np.iinfo(np.int64).max
FIGURES = ("pixels", "vertices", "faces", "wall_faces", "crossing_walls", "top_min", "top_max", "volume6")
TOTALS = ("n_pixels", "n_vertices", "n_faces", "n_indices", "n_wall_faces", "n_crossing_walls", "total_volume6")
MESH = ("vertex", "face_offset", "face_index", "face_building", "face_kind")
# wall d: s and e as top components k = 2 j + i of the pixel, the neighbour's offset (dx, dy), and the components of the
# neighbour that sit at s and e
WALLS = ((0, 1, (0, -1), 2, 3), (1, 3, (1, 0), 0, 2), (3, 2, (0, 1), 1, 0), (2, 0, (-1, 0), 3, 1))


def tops(bmap, roof, normal, center, z_min, z_max, bin, base_z, flat):
    """top int32 [height][width][4] = {t00, t10, t01, t11}, I32_MIN x 4 outside every building"""
    bmap, roof = np.asarray(bmap, np.int64), np.asarray(roof, np.int64)
    h, w = bmap.shape
    top = np.full((h, w, 4), I32_MIN, np.int64)
    inb = bmap >= 0
    fl = np.asarray(flat, np.int64).reshape(-1)
    un = inb & (roof <= 0)
    top[un] = np.maximum(base_z, fl[bmap[un]])[:, None]
    ys, xs = np.nonzero(inb & (roof > 0))
    if len(ys):
        p = roof[ys, xs]
        for k in range(4):
            z = rr.height_of(p, (xs + (k & 1)) * bin, (ys + (k >> 1)) * bin, normal, center, z_min, z_max)
            top[ys, xs, k] = np.maximum(base_z, z)
    return top.astype(np.int32)


def _corner_keys(bmap, top, base_z):
    """sorted keys [height + 1][width + 1][8] (building << 32 | height + 2^31, NO_KEY last) and the flags of the distinct"""
    h, w = bmap.shape
    m = np.full((h + 2, w + 2), -1, np.int64)
    m[1:-1, 1:-1] = bmap
    t = np.zeros((h + 2, w + 2, 4), np.int64)
    t[1:-1, 1:-1] = top
    keys = np.full((h + 1, w + 1, 8), NO_KEY, np.int64)
    for q in range(4):  # incident pixel (X - 1 + (q & 1), Y - 1 + (q >> 1)); the corner is its component 3 - q
        dy, dx = q >> 1, q & 1
        c = m[dy:dy + h + 1, dx:dx + w + 1]
        z = t[dy:dy + h + 1, dx:dx + w + 1, 3 - q]
        ok = c >= 0
        keys[..., 2 * q] = np.where(ok, (c << 32) | (base_z + 2 ** 31), NO_KEY)
        keys[..., 2 * q + 1] = np.where(ok, (c << 32) | (z + 2 ** 31), NO_KEY)
    keys.sort(axis=-1)
    distinct = keys != NO_KEY
    distinct[..., 1:] &= keys[..., 1:] != keys[..., :-1]
    return keys, distinct


def solids(bmap, roof, n_buildings, normal, center, z_min, z_max, bin, base_z, flat):
    bmap = np.asarray(bmap, np.int64)
    bmap = np.where(bmap < 0, -1, bmap)
    h, w = bmap.shape
    nb, base_z = int(n_buildings), int(base_z)
    top32 = tops(bmap, roof, normal, center, z_min, z_max, bin, base_z, flat)
    top = top32.astype(np.int64)
    keys, distinct = _corner_keys(bmap, top, base_z)
    cnt = distinct.sum(-1)
    voff = np.zeros(cnt.size + 1, np.int64)
    voff[1:] = np.cumsum(cnt.ravel())
    voff = voff[:-1].reshape(h + 1, w + 1)
    rank = np.cumsum(distinct, -1) - 1
    # vertices in (Y, X, c, Z) order: the distinct keys in array order
    Yc, Xc, Kc = np.nonzero(distinct)
    kv = keys[Yc, Xc, Kc]
    vertex = np.stack([Xc * bin, Yc * bin, (kv & 0xFFFFFFFF) - 2 ** 31, kv >> 32], 1).astype(np.int32)

    ys, xs = np.nonzero(bmap >= 0)  # row-major
    n = len(ys)
    c = bmap[ys, xs]
    T = top[ys, xs]
    key_c = c << 32

    def vid(k, z, sel=slice(None)):
        """vertex number of (corner k of the pixels `sel`, height z)"""
        Y, X = ys[sel] + (k >> 1), xs[sel] + (k & 1)
        key = key_c[sel] | (z + 2 ** 31)
        return voff[Y, X] + ((keys[Y, X] < key[:, None]) & distinct[Y, X]).sum(1)

    tv = [vid(k, T[:, k]) for k in range(4)]
    bv = [vid(k, np.full(n, base_z, np.int64)) for k in range(4)]
    pix = np.arange(n, dtype=np.int64)
    # every face as a row of up to 8 vertex numbers (-1: none) with the sort key pixel * 7 + slot
    rows = [np.stack([tv[0], tv[1], tv[3]], 1), np.stack([tv[0], tv[3], tv[2]], 1), np.stack([bv[0], bv[2], bv[3], bv[1]], 1)]
    slots, kinds, who = [pix * 7, pix * 7 + 1, pix * 7 + 2], [0, 0, 1], [pix, pix, pix]
    walls = np.zeros(n, np.int64)
    crossing = np.zeros(n, np.int64)
    mp = np.full((h + 2, w + 2), -1, np.int64)
    mp[1:-1, 1:-1] = bmap
    tp = np.zeros((h + 2, w + 2, 4), np.int64)
    tp[1:-1, 1:-1] = top
    for d, (ks, ke, (dx, dy), ns, ne) in enumerate(WALLS):
        same = mp[ys + 1 + dy, xs + 1 + dx] == c
        a_s, a_e = T[:, ks], T[:, ke]
        b_s = np.where(same, tp[ys + 1 + dy, xs + 1 + dx, ns], base_z)
        b_e = np.where(same, tp[ys + 1 + dy, xs + 1 + dx, ne], base_z)
        exists = ((a_s != b_s) | (a_e != b_e)) & ~(same & (d in (0, 3)))
        sel = np.nonzero(exists)[0]
        if not len(sel):
            continue
        a_s, a_e, b_s, b_e = a_s[sel], a_e[sel], b_s[sel], b_e[sel]
        walls[sel] += 1
        crossing[sel] += ((a_s > b_s) & (a_e < b_e)) | ((a_s < b_s) & (a_e > b_e))
        kc = key_c[sel]

        def side(k, z_from, z_to):
            """the vertices of corner k strictly between the two heights, walking from z_from: [m][8] with -1 padding"""
            Y, X = ys[sel] + (k >> 1), xs[sel] + (k & 1)
            K, D = keys[Y, X], distinct[Y, X]
            lo = kc | (np.minimum(z_from, z_to) + 2 ** 31)
            hi = kc | (np.maximum(z_from, z_to) + 2 ** 31)
            mid = D & (K > lo[:, None]) & (K < hi[:, None])
            ids = np.where(mid, voff[Y, X][:, None] + rank[Y, X], -1)
            down = z_from > z_to
            ids[down] = ids[down, ::-1]
            return ids

        one = lambda a, keep=None: np.where(keep, a, -1)[:, None] if keep is not None else a[:, None]  # noqa: E731
        poly = np.concatenate([one(tv[ke][sel]), one(tv[ks][sel]), side(ks, a_s, b_s), one(vid(ks, b_s, sel), a_s != b_s),
                               one(vid(ke, b_e, sel), a_e != b_e), side(ke, b_e, a_e)], 1)
        order = np.argsort(poly < 0, axis=1, kind="stable")  # the kept ones first, in order
        poly = np.take_along_axis(poly, order, 1)[:, :8]
        rows.append(poly)
        slots.append(sel * 7 + 3 + d)
        kinds.append(2)
        who.append(sel)
    nfaces = sum(len(r) for r in rows)
    F = np.full((nfaces, 8), -1, np.int64)
    at = 0
    for r in rows:
        F[at:at + len(r), :r.shape[1]] = r
        at += len(r)
    slot = np.concatenate(slots) if n else np.zeros(0, np.int64)
    kind = np.concatenate([np.full(len(s), k, np.uint8) for s, k in zip(slots, kinds)]) if n else np.zeros(0, np.uint8)
    owner = np.concatenate([c[p] for p in who]) if n else np.zeros(0, np.int64)
    order = np.argsort(slot, kind="stable")
    F, kind, owner = F[order], kind[order], owner[order]
    keep = F >= 0
    off = np.zeros(nfaces + 1, np.int64)
    off[1:] = np.cumsum(keep.sum(1))
    assert nfaces == 0 or (3 <= keep.sum(1).min() and keep.sum(1).max() <= 8)

    def per(wt):
        return np.bincount(c, weights=None if wt is None else wt, minlength=nb)[:nb].astype(np.int64)

    fig = dict(pixels=per(None), faces=np.bincount(c, 3 + walls, nb).astype(np.int64) if n else np.zeros(nb, np.int64),
               wall_faces=np.bincount(c, walls, nb).astype(np.int64) if n else np.zeros(nb, np.int64),
               crossing_walls=np.bincount(c, crossing, nb).astype(np.int64) if n else np.zeros(nb, np.int64),
               vertices=np.bincount(vertex[:, 3], minlength=nb).astype(np.int64))
    tmin, tmax = np.full(nb, I32_MAX, np.int64), np.full(nb, I32_MIN, np.int64)
    np.minimum.at(tmin, c, T.min(1))
    np.maximum.at(tmax, c, T.max(1))
    vol = np.zeros(nb, np.int64)
    np.add.at(vol, c, 2 * T[:, 0] + 2 * T[:, 3] + T[:, 1] + T[:, 2] - 6 * base_z)
    fig.update(top_min=tmin.astype(np.int32), top_max=tmax.astype(np.int32), volume6=vol)
    return SimpleNamespace(
        top=top32, vertex=vertex, face_offset=off.astype(np.int32), face_index=F[keep].astype(np.int32),
        face_building=owner.astype(np.int32), face_kind=kind, n_buildings=nb, n_pixels=n, n_vertices=len(vertex),
        n_faces=nfaces, n_indices=int(off[-1]), n_wall_faces=int(walls.sum()), n_crossing_walls=int(crossing.sum()),
        total_volume6=int(vol.sum()), **fig)


def same(a, b, names=("top",) + MESH + FIGURES + TOTALS):
    """the first name in which two results differ, or None"""
    for k in names:
        x, y = getattr(a, k), getattr(b, k)
        if isinstance(y, np.ndarray):
            if not (isinstance(x, np.ndarray) and x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)):
                return k
        elif int(x) != int(y):
            return k
    return None


def _face_corners(m):
    """(face of every index, position of the index inside its face, the index of the next vertex of the same face)"""
    off = np.asarray(m.face_offset, np.int64)
    ln = np.diff(off)
    face = np.repeat(np.arange(len(ln)), ln)
    pos = np.arange(off[-1]) - off[face]
    nxt = off[face] + (pos + 1) % ln[face]
    return face, pos, nxt


def unmatched_edges(m):
    """property (a) from the arrays alone: the number of directed edges (u, v) whose count differs from that of (v, u),
    counted per building (an edge never pairs with one of another building: vertices carry their building)"""
    idx = np.asarray(m.face_index, np.int64)
    if not len(idx):
        return 0
    _, _, nxt = _face_corners(m)
    u, v = idx, idx[nxt]
    nv = len(m.vertex)
    both, inv = np.unique(np.concatenate([u * nv + v, v * nv + u]), return_inverse=True)
    net = np.bincount(inv, np.concatenate([np.ones(len(u)), -np.ones(len(u))]), len(both))
    return int((net != 0).sum())


def det_sums(m, n_buildings):
    """property (b) from the arrays alone: per building the sum of det(v0, vk, vk+1) over the fan triangles of its faces
    (millimetres; int64, exact modulo 2^64)"""
    out = np.zeros(n_buildings, np.int64)
    idx = np.asarray(m.face_index, np.int64)
    if not len(idx):
        return out
    off = np.asarray(m.face_offset, np.int64)
    face, pos, nxt = _face_corners(m)
    ln = np.diff(off)
    use = (pos >= 1) & (pos < ln[face] - 1)  # k = 1 .. len - 2: triangle (0, k, k + 1)
    P = np.asarray(m.vertex, np.int64)[:, :3]
    a, b, c = P[idx[off[face[use]]]], P[idx[use]], P[idx[nxt[use]]]
    with np.errstate(over="ignore"):
        det = (a * np.cross(b, c)).sum(1)
        np.add.at(out, np.asarray(m.face_building, np.int64)[face[use]], det)
    return out


def obj_text(m, origin=None):
    """the file of bs_solids_write_obj (include/bs_api.h) as bytes"""
    o = np.zeros(3, np.int64) if origin is None else np.asarray(origin, np.int64)
    fb = np.asarray(m.face_building, np.int64)
    used = np.unique(fb)
    out = [f"# solids: {len(used)} buildings, {len(m.vertex)} vertices, {len(fb)} faces\n"]
    P = np.asarray(m.vertex, np.int64)[:, :3] + o
    out += [f"v {x} {y} {z}\n" for x, y, z in P.tolist()]
    off, idx = np.asarray(m.face_offset).tolist(), (np.asarray(m.face_index, np.int64) + 1).tolist()
    for c in used.tolist():
        out.append(f"o building_{c}\n")
        for f in np.nonzero(fb == c)[0].tolist():
            out.append("f " + " ".join(map(str, idx[off[f]:off[f + 1]])) + "\n")
    return "".join(out).encode()


def parse_obj(data, n_buildings_hint=None):
    """the mesh arrays back from an OBJ of bs_solids_write_obj (the faces come back grouped by building, the vertex's
    building column from the faces that use it)"""
    vs, off, idx, fb, cur = [], [0], [], [], -1
    for ln in data.decode().splitlines():
        t = ln.split()
        if t[0] == "v":
            vs.append([int(t[1]), int(t[2]), int(t[3]), -1])
        elif t[0] == "o":
            cur = int(t[1].split("_")[1])
        elif t[0] == "f":
            idx += [int(k) - 1 for k in t[1:]]
            off.append(len(idx))
            fb.append(cur)
    return SimpleNamespace(vertex=np.array(vs, np.int64).reshape(-1, 4), face_offset=np.array(off, np.int64),
                           face_index=np.array(idx, np.int64), face_building=np.array(fb, np.int64))
