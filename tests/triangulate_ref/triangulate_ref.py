"""Outline triangles (include/bs_api.h, "outline triangles") as the device computes them, restated in numpy: per label
its rings, vertices V, holes H and outer rings O, its occurrences V + 2 H, its first triangle and its bin (a wave up to
WAVE_CAP occurrences, a workgroup with its slots in LDS up to LDS_CAP, a workgroup with a global workspace beyond); the
leftmost vertex of every hole by two minima; per label the slot arrays (x, y, next, prev, the label-local vertex with the
flags "in a list" and "in the current list, not clipped"), slot i < V vertex vbase + i, slots V + 2 j and V + 2 j + 1 the
second occurrences M', V' of the j-th bridge; the candidates of a bridge by ascending (d2, vertex, slot) with the cones first
and the blockers -- the edges slot -> next[slot] of every slot in use -- only for the least one left; the ear scan with every
slot of the current list a blocker.  tests/triangulate_ref/brute.py is the definition; the two must be equal."""
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


brute = _load("triangulate_brute", os.path.join(HERE, "brute.py"))
uref = brute.uref

WAVE_CAP, LDS_CAP = 64, 1024  # BS_TRI_WAVE_CAP, BS_TRI_LDS_CAP of include/bs_api.h
PATHS = ("n_labels_wave", "n_labels_lds", "n_labels_global")
DEVICE_FIELDS = brute.FIELDS + PATHS  # what the device and the restatement share
OK, NO_BRIDGE, STALLED, EMPTY = brute.OK, brute.NO_BRIDGE, brute.STALLED, brute.EMPTY


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _in_cone(px, py, vx, vy, nx, ny, dx, dy):
    ax, ay, qx, qy = nx - vx, ny - vy, px - vx, py - vy
    convex = _orient(px, py, vx, vy, nx, ny) > 0
    return np.where(convex, (ax * dy - ay * dx > 0) & (dx * qy - dy * qx > 0), ~((qx * dy - qy * dx >= 0) & (dx * ay - dy * ax >= 0)))


def _blocks(sx, sy, ex, ey, M, V):
    (mx, my), (vx, vy) = M, V
    o1, o2 = _orient(mx, my, vx, vy, sx, sy), _orient(mx, my, vx, vy, ex, ey)
    o3, o4 = _orient(sx, sy, ex, ey, mx, my), _orient(sx, sy, ex, ey, vx, vy)
    proper = (((o1 > 0) & (o2 < 0)) | ((o1 < 0) & (o2 > 0))) & (((o3 > 0) & (o4 < 0)) | ((o3 < 0) & (o4 > 0)))

    def box(ax, ay, bx, by, px, py):
        return (px >= np.minimum(ax, bx)) & (px <= np.maximum(ax, bx)) & (py >= np.minimum(ay, by)) & (py <= np.maximum(ay, by))

    def at(px, py, Q):
        return (px == Q[0]) & (py == Q[1])

    t1 = (o1 == 0) & ~at(sx, sy, M) & ~at(sx, sy, V) & box(mx, my, vx, vy, sx, sy)
    t2 = (o2 == 0) & ~at(ex, ey, M) & ~at(ex, ey, V) & box(mx, my, vx, vy, ex, ey)
    t3 = (o3 == 0) & ~at(sx, sy, M) & ~at(ex, ey, M) & box(sx, sy, ex, ey, mx, my)
    t4 = (o4 == 0) & ~at(sx, sy, V) & ~at(ex, ey, V) & box(sx, sy, ex, ey, vx, vy)
    return proper | t1 | t2 | t3 | t4


def _label(X, Y, soff, outer, rm, r0, r1, trace=None):
    """one work item: returns (status, triangles as global vertices, {ring: (M, V)}, tests)"""
    vb = int(soff[r0])
    V = int(soff[r1]) - vb
    H = int((~outer[r0:r1]).sum())
    nocc = V + 2 * H
    px, py = np.zeros(nocc, np.int64), np.zeros(nocc, np.int64)
    px[:V], py[:V] = X[vb:vb + V], Y[vb:vb + V]
    s = np.arange(V)
    ring = np.repeat(np.arange(r0, r1), np.diff(soff[r0:r1 + 1]))
    a, b = soff[ring] - vb, soff[ring + 1] - vb
    nx, pv = np.arange(nocc), np.arange(nocc)
    nx[:V], pv[:V] = np.where(s + 1 < b, s + 1, a), np.where(s > a, s - 1, b - 1)
    vt = np.zeros(nocc, np.int64)
    vt[:V] = s
    inl = np.zeros(nocc, bool)
    inl[:V] = outer[ring]
    bridges = {}
    # ---- bridges: the holes by ascending (x, y, vertex) of their leftmost vertex
    holes = [r for r in range(r0, r1) if not outer[r]]
    holes.sort(key=lambda r: (int(X[rm[r]]), int(Y[rm[r]]), int(rm[r])))
    for j, r in enumerate(holes):
        m = int(rm[r]) - vb
        used = V + 2 * j
        M = (int(px[m]), int(py[m]))
        mp, mn = int(pv[m]), int(nx[m])
        u = np.arange(used)
        cand = u[inl[:used] & ~((px[:used] == M[0]) & (py[:used] == M[1]))]
        dx, dy = M[0] - px[cand], M[1] - py[cand]
        cone = (_in_cone(px[pv[cand]], py[pv[cand]], px[cand], py[cand], px[nx[cand]], py[nx[cand]], dx, dy) &
                _in_cone(px[mp], py[mp], M[0], M[1], px[mn], py[mn], -dx, -dy))
        cand, d2 = cand[cone], (dx * dx + dy * dy)[cone]
        order = np.lexsort((cand, vt[cand], d2))
        pick = -1
        for c in cand[order].tolist():  # the blockers of the least candidate left
            if not _blocks(px[:used], py[:used], px[nx[:used]], py[nx[:used]], M, (int(px[c]), int(py[c]))).any():
                pick = c
                break
            if trace is not None:
                trace["blocked_candidates"] = trace.get("blocked_candidates", 0) + 1
        if pick < 0:
            return NO_BRIDGE, [], {}, 0
        c, d0, d1 = pick, used, used + 1
        on, cv = int(nx[c]), int(vt[c])
        inl[soff[r] - vb:soff[r + 1] - vb] = True
        nx[c], pv[m] = m, c
        nx[mp], pv[d0], nx[d0], pv[d1], nx[d1], pv[on] = d0, mp, d1, d0, on, d1
        px[d0], py[d0], vt[d0], px[d1], py[d1], vt[d1] = M[0], M[1], m, px[c], py[c], cv
        inl[d0] = inl[d1] = True
        bridges[r] = (vb + m, vb + cv)
    # ---- ears
    tris, tests = [], 0
    nxl, pvl, pxl, pyl, vtl = nx.tolist(), pv.tolist(), px.tolist(), py.tolist(), vt.tolist()
    n_outer = (r1 - r0) - H
    for r in range(r0, r1):
        if not outer[r]:
            continue
        start = int(soff[r]) - vb
        cur_flag = np.zeros(nocc, bool)
        if n_outer == 1:
            cur_flag[:] = inl
        else:
            q = start
            while True:
                cur_flag[q] = True
                q = nxl[q]
                if q == start:
                    break
        left = int(cur_flag.sum())
        cur = stop = start
        while left > 3:
            b_, a_, c_ = cur, pvl[cur], nxl[cur]
            ax, ay, bx, by, cx, cy = pxl[a_], pyl[a_], pxl[b_], pyl[b_], pxl[c_], pyl[c_]
            tests += 1
            ear = _orient(ax, ay, bx, by, cx, cy) > 0
            if ear:
                q = np.flatnonzero(cur_flag)
                qx, qy = px[q], py[q]
                other = ~(((qx == ax) & (qy == ay)) | ((qx == bx) & (qy == by)) | ((qx == cx) & (qy == cy)))
                ear = not (other & (_orient(ax, ay, bx, by, qx, qy) >= 0) & (_orient(bx, by, cx, cy, qx, qy) >= 0) &
                           (_orient(cx, cy, ax, ay, qx, qy) >= 0)).any()
            if ear:
                tris.append((vb + vtl[a_], vb + vtl[b_], vb + vtl[c_]))
                nxl[a_], pvl[c_] = c_, a_
                cur_flag[b_] = False
                left -= 1
                cur = stop = nxl[c_]
            else:
                cur = c_
                if cur == stop:
                    return STALLED, [], {}, tests
        tris.append((vb + vtl[pvl[cur]], vb + vtl[cur], vb + vtl[nxl[cur]]))
    return OK, tris, bridges, tests


def triangulate(plain, clean, trace=None):
    """the outline triangles of the clean outlines `clean` over the plain outlines `plain` (of uncross_ref.clean); trace: a
    dict that receives the candidates of bridges that passed the cones and were blocked"""
    nl, nr = int(plain.n_labels), int(clean.n_rings)
    sxy = np.asarray(clean.sxy, np.int64).reshape(-1, 2)
    X, Y = sxy[:, 0], sxy[:, 1]
    nsv = len(X)
    soff = np.asarray(clean.s_ring_offset, np.int64)
    lro = np.asarray(plain.label_ring_offset, np.int64)
    outer = np.asarray(plain.ring_area2, np.int64)[:nr] > 0
    # the prologue: per label V, H, O, occurrences, triangles, bins
    rv = np.diff(soff)
    cs = lambda v: np.concatenate([[0], np.cumsum(v)])  # noqa: E731
    Vl = cs(rv)[lro[1:]] - cs(rv)[lro[:-1]]
    Hl = cs(~outer)[lro[1:]] - cs(~outer)[lro[:-1]]
    Ol = cs(outer)[lro[1:]] - cs(outer)[lro[:-1]]
    occ = Vl + 2 * Hl
    ntri = np.where(lro[1:] > lro[:-1], occ - 2 * Ol, 0)
    tri_offset = cs(ntri)
    has = lro[1:] > lro[:-1]
    paths = (int((has & (occ <= WAVE_CAP)).sum()), int((has & (occ > WAVE_CAP) & (occ <= LDS_CAP)).sum()), int((has & (occ > LDS_CAP)).sum()))
    # the leftmost vertex of every hole: two minima
    ringv = np.repeat(np.arange(nr), rv)
    key = (X << 32) | Y
    rkey = np.full(nr, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(rkey, ringv, key)
    rm = np.full(nr, np.iinfo(np.int64).max, np.int64)
    at = key == rkey[ringv]
    np.minimum.at(rm, ringv[at], np.arange(nsv)[at])
    tri = np.full((int(tri_offset[-1]), 3), -1, np.int32)
    status = np.full(nl, EMPTY, np.int32)
    area2, tests = np.zeros(nl, np.int64), np.zeros(nl, np.int64)
    bridge = np.full((nr, 2), -1, np.int32)
    for l in np.flatnonzero(has).tolist():
        st, t, br, nt = _label(X, Y, soff, outer, rm, int(lro[l]), int(lro[l + 1]), trace)
        status[l], tests[l] = st, nt
        if st == OK:
            assert len(t) == ntri[l]
            t = np.array(t, np.int64).reshape(-1, 3)
            tri[tri_offset[l]:tri_offset[l + 1]] = t
            area2[l] = _orient(X[t[:, 0]], Y[t[:, 0]], X[t[:, 1]], Y[t[:, 1]], X[t[:, 2]], Y[t[:, 2]]).sum()
            for r, mv in br.items():
                bridge[r] = mv
    return SimpleNamespace(
        n_labels=nl, tri=tri, tri_offset=tri_offset.astype(np.int64), bridge=bridge, label_status=status, label_area2=area2,
        label_tests=tests, n_triangles=int(tri_offset[-1]), n_failed_labels=int(((status == NO_BRIDGE) | (status == STALLED)).sum()),
        n_bridges=int((bridge[:, 0] >= 0).sum()), n_tests=int(tests.sum()), max_label_occurrences=int(occ.max()) if nl else 0,
        n_labels_wave=paths[0], n_labels_lds=paths[1], n_labels_global=paths[2])


def same(a, b, fields=DEVICE_FIELDS):
    return brute.same(a, b, fields)
