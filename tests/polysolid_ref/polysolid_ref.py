"""Polygon solids (include/bs_api.h, "polygon solids") as the device computes them, restated in vectorised numpy: per label
its building (-1 where that is open), its first vertex and the triangles up to and including it; the twins by one stable sort
of the keys (lower corner << 32 | higher corner) of the segments that have their own building on their right, positions 2 k
and 2 k + 1 a pair; the vertex numbers by a stable sort of the two entries (building, corner, Z) of every clean vertex of a
closed building, head flags and their running sum; the walls from differences of vertex numbers; the offsets by exclusive
sums.  tests/polysolid_ref/brute.py is the definition; the two must be equal."""
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


brute = _load("polysolid_brute", os.path.join(HERE, "brute.py"))
tref, tbrute, uref = brute.tref, brute.tbrute, brute.uref

FIG_CAP = 1024  # BS_POLY_FIG_CAP of include/bs_api.h
FIELDS = brute.FIELDS


def _cs(v):
    return np.concatenate([[0], np.cumsum(v)]).astype(np.int64)


def poly_solids(plain, clean, tri, label_building, n_buildings, bin, base_z, trace=None):
    """the polygon solids over the triangles `tri` of the clean outlines `clean` (with sz) over the plain outlines `plain`;
    trace: a dict that receives what the regimes of tests/polysolid_ref/cases.py need"""
    nl, nb = int(tri.n_labels), int(n_buildings)
    lb = np.asarray(label_building, np.int64).reshape(-1)
    assert len(lb) == nl and ((lb >= 0) & (lb < nb)).all()
    sxy = np.asarray(clean.sxy, np.int64).reshape(-1, 2)
    X, Y = sxy[:, 0], sxy[:, 1]
    nsv = len(X)
    Z = np.asarray(clean.sz, np.int64).reshape(-1) if nsv else np.zeros(0, np.int64)
    right = np.asarray(clean.s_right, np.int64).reshape(-1)
    soff = np.asarray(clean.s_ring_offset, np.int64)
    lro = np.asarray(plain.label_ring_offset, np.int64)
    status = np.asarray(tri.label_status, np.int64)
    toff = np.asarray(tri.tri_offset, np.int64)
    T = np.asarray(tri.tri, np.int64).reshape(-1, 3)
    nr = len(soff) - 1
    assert (np.abs(Z - base_z) < brute.Z_LIMIT).all()
    # the host's part
    failed = (status == tbrute.NO_BRIDGE) | (status == tbrute.STALLED)
    is_open = np.zeros(nb, np.int64)
    is_open[lb[failed]] = 1
    lc = np.where(is_open[lb] == 1, -1, lb) if nl else np.zeros(0, np.int64)
    contributes = (lc >= 0) & (status == tbrute.OK)
    tb2 = np.cumsum(np.where(contributes, np.diff(toff), 0)) if nl else np.zeros(0, np.int64)
    lv0 = soff[lro[:-1]]
    rlabel = np.repeat(np.arange(nl), np.diff(lro))
    fig = {k: np.zeros(nb, np.int64) for k in brute.FIGURES}
    fig["status"] = is_open
    fig["labels"] = np.bincount(lb, minlength=nb).astype(np.int64)
    fig["roof_faces"] = np.bincount(lb[contributes], weights=np.diff(toff)[contributes], minlength=nb).astype(np.int64)
    fig["z_min"], fig["z_max"] = np.full(nb, brute.INT32_MAX, np.int64), np.full(nb, brute.INT32_MIN, np.int64)
    tb = int(tb2[-1]) if nl else 0
    if nsv == 0:
        return brute.pack(nb, [], [], {k: v.tolist() for k, v in fig.items()})
    ring = np.repeat(np.arange(nr), np.diff(soff))
    i = np.arange(nsv)
    nxt = np.where(i + 1 < soff[ring + 1], i + 1, soff[ring])
    lab = rlabel[ring]
    c = lc[lab]
    corner = Y * (int(X.max()) + 1) + X
    # 1. twins
    need = (c >= 0) & (right >= 0)
    need[need] = lc[right[need]] == c[need]
    key = (np.minimum(corner, corner[nxt]) << 32) | np.maximum(corner, corner[nxt])
    s = np.flatnonzero(need)
    s = s[np.argsort(key[s], kind="stable")]
    assert len(s) % 2 == 0, "a twin is missing"
    a, b = s[0::2], s[1::2]
    assert (key[a] == key[b]).all() and (right[a] == lab[b]).all() and (right[b] == lab[a]).all()
    assert (corner[a] == corner[nxt[b]]).all() and (corner[nxt[a]] == corner[b]).all()
    twin = np.full(nsv, -1, np.int64)
    twin[a], twin[b] = b, a
    # 2. vertices: entry 2 i is (c, corner, Z[i]), entry 2 i + 1 is (c, corner, base_z)
    ez = np.stack([Z, np.full(nsv, base_z, np.int64)], 1).reshape(-1)
    ecol = np.repeat((c << 32) | corner, 2)
    valid = np.flatnonzero(np.repeat(c >= 0, 2))
    order = valid[np.lexsort((ez[valid], ecol[valid]))]
    head = np.ones(len(order), bool)
    head[1:] = (ecol[order][1:] != ecol[order][:-1]) | (ez[order][1:] != ez[order][:-1])
    vnum = np.full(2 * nsv, -1, np.int64)
    vnum[order] = np.cumsum(head) - 1
    src = order[head]
    vc = ecol[src] >> 32
    vertex = np.stack([X[src >> 1] * bin, Y[src >> 1] * bin, ez[src], vc], 1)
    nv = len(src)
    fig["vertices"] = np.bincount(vc, minlength=nb).astype(np.int64)
    # 3. count: the wall of every segment
    has = twin >= 0
    tw = np.where(has, twin, 0)
    va_s, va_e = vnum[2 * i], vnum[2 * nxt]
    vb_s = np.where(has, vnum[2 * nxt[tw]], vnum[2 * i + 1])
    vb_e = np.where(has, vnum[2 * tw], vnum[2 * nxt + 1])
    b_s, b_e = np.where(has, Z[nxt[tw]], base_z), np.where(has, Z[tw], base_z)
    ds, de = np.abs(va_s - vb_s), np.abs(va_e - vb_e)
    emit = (c >= 0) & (ds + de > 0) & (~has | (lab < lab[tw]))
    wcnt = np.where(emit, 2 + ds + de, 0)
    crossing = emit & ((Z - b_s) * (Z[nxt] - b_e) < 0)
    wscan, iscan = _cs(emit), _cs(wcnt)
    cl = np.where(c >= 0, c, 0)
    used = c >= 0
    fig["wall_faces"] = np.bincount(cl[emit], minlength=nb).astype(np.int64)
    fig["crossing_walls"] = np.bincount(cl[crossing], minlength=nb).astype(np.int64)
    np.maximum.at(fig["max_wall_vertices"], cl[emit], wcnt[emit])
    np.minimum.at(fig["z_min"], cl[used], Z[used])
    np.maximum.at(fig["z_max"], cl[used], Z[used])
    fig["faces"] = 2 * fig["roof_faces"] + fig["wall_faces"]
    nf, ni = 2 * tb + int(wscan[-1]), 6 * tb + int(iscan[-1])
    # the triangles of the contributing labels
    ql = np.repeat(np.arange(nl), np.diff(toff))
    q = np.flatnonzero(contributes[ql])
    ql = ql[q]
    ta, tb_, td = T[q, 0], T[q, 1], T[q, 2]
    o = (X[tb_] - X[ta]) * (Y[td] - Y[ta]) - (Y[tb_] - Y[ta]) * (X[td] - X[ta])
    qc = lc[ql]
    np.add.at(fig["area2"], qc, o)
    np.add.at(fig["volume6"], qc, o * (Z[ta] + Z[tb_] + Z[td] - 3 * base_z))
    # 4. emit
    offset, index = np.zeros(nf + 1, np.int64), np.full(ni, -1, np.int64)
    building, kind = np.full(nf, -1, np.int64), np.full(nf, 255, np.int64)
    offset[nf] = ni
    Tl = np.diff(toff)[ql]
    tbl = tb2[ql] - Tl
    j = q - toff[ql]
    F, I = 2 * tbl + wscan[lv0[ql]], 6 * tbl + iscan[lv0[ql]]
    f0, f1, i0, i1 = F + j, F + Tl + j, I + 3 * j, I + 3 * Tl + 3 * j
    offset[f0], offset[f1] = i0, i1
    building[f0] = building[f1] = qc
    kind[f0], kind[f1] = 0, 1
    index[i0], index[i0 + 1], index[i0 + 2] = vnum[2 * ta], vnum[2 * tb_], vnum[2 * td]
    index[i1], index[i1 + 1], index[i1 + 2] = vnum[2 * td + 1], vnum[2 * tb_ + 1], vnum[2 * ta + 1]
    w = np.flatnonzero(emit)
    f, k = 2 * tb2[lab[w]] + wscan[w], 6 * tb2[lab[w]] + iscan[w]
    offset[f], building[f], kind[f] = k, c[w], 2
    index[k], index[k + 1] = va_e[w], va_s[w]
    ss, se = np.where(vb_s[w] > va_s[w], 1, -1), np.where(va_e[w] > vb_e[w], 1, -1)
    for step in range(1, int(ds[w].max()) + 1 if len(w) else 0):
        m = ds[w] >= step
        index[k[m] + 1 + step] = va_s[w][m] + step * ss[m]
    for step in range(int(de[w].max()) if len(w) else 0):
        m = de[w] > step
        index[k[m] + 2 + ds[w][m] + step] = vb_e[w][m] + step * se[m]
    assert (index >= 0).all() and (building >= 0).all() and (kind < 3).all()
    if trace is not None:
        trace.update(wall_sizes=sorted(set(wcnt[emit].tolist())), n_twin_walls=int((emit & has).sum()),
                     n_base_walls=int((emit & ~has).sum()), n_suppressed=int(((c >= 0) & has & (ds + de > 0) & ~emit).sum()),
                     n_flush=int(((c >= 0) & (ds + de == 0)).sum()), between_up=int((emit & (ds > 1) & (vb_s > va_s)).sum()),
                     between_down=int((emit & (ds > 1) & (vb_s < va_s)).sum()), below_base=int((used & (Z < base_z)).sum()),
                     other_building=int(((c >= 0) & (right >= 0) & ~need).sum()), outside=int(((c >= 0) & (right < 0)).sum()),
                     column_max=int(np.unique(ecol[src], return_counts=True)[1].max()) if nv else 0,
                     columns_of_5=int((np.unique(ecol[src], return_counts=True)[1] == 5).sum()) if nv else 0)
    out = brute.pack(nb, [], [], {k: v.tolist() for k, v in fig.items()})
    out.vertex = vertex.astype(np.int32).reshape(nv, 4)
    out.face_offset, out.face_index = offset.astype(np.int32), index.astype(np.int32)
    out.face_building, out.face_kind = building.astype(np.int32), kind.astype(np.uint8)
    out.n_vertices, out.n_faces, out.n_indices = nv, nf, ni
    return out


def same(a, b, fields=FIELDS):
    return brute.same(a, b, fields)
