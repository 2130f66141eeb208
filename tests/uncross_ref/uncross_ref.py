"""Clean outlines (include/bs_api.h, "clean outlines") as the device computes them, restated in numpy: the node arrays of
the simplified stage in the rotated order and its kept flags; per round the kept flags scanned and listed, the segments
(left kept node, right kept node across the ring's wrap), the cells every segment touches column of cells by column, the
(cell, segment) entries sorted by cell, the pair tests of every cell's run, the marks; the nodes of marked segments
activated with their spanning segment and one forced round (greatest c^2, lowest corner); the un-rotation of the final
kept nodes with their flags.  tests/uncross_ref/brute.py tests all pairs instead; the two must be equal."""
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


sref = _load("simplify_ref", os.path.join(HERE, "..", "simplify_ref", "simplify_ref.py"))
brute = _load("uncross_brute", os.path.join(HERE, "brute.py"))
orf = sref.orf

DEFAULT_CELL_LOG2 = 4
DEVICE_FIELDS = brute.FIELDS + ("n_entries", "max_cell_entries")  # what the device and the restatement share
NO_TIE = (1 << 63) - 1


def node_arrays(label, top, n_labels):
    """the node arrays of tests/simplify_ref/simplify_ref.py in the rotated order"""
    h, w = label.shape
    tr = {}
    plain = orf.outlines(label, top, n_labels, trace=tr)
    succ, vert, leader, hnum, R = tr["succ"], tr["vert"], tr["leader"], tr["hnum"], tr["R"]
    n = len(hnum)
    p, k = hnum >> 2, hnum & 3
    x, y = p % w, p // w
    X, Y = x + orf.SX[k], y + orf.SY[k]
    L = np.pad(np.maximum(label, -1), 1, constant_values=-1)
    a, b, c, d = L[Y, X], L[Y, X + 1], L[Y + 1, X], L[Y + 1, X + 1]
    distinct = 1 + (b != a) + ((c != a) & (c != b)) + ((d != a) & (d != b) & (d != c))
    junction = (distinct >= 3) | ((a == d) & (b == c) & (a != b))
    node = vert | junction
    right = L[y + orf.DY[k] + 1, x + orf.DX[k] + 1]
    cidx = Y * (w + 1) + X
    zn = np.asarray(top)[y, x, orf.ZIDX[k]] if top is not None else np.zeros(n, np.int64)
    nxt = np.where(succ == leader, -1, succ)
    val = node.astype(np.int64)
    for _ in range(R):
        live = nxt != -1
        j = np.where(live, nxt, 0)
        val, nxt = np.where(live, val + val[j], val), np.where(live, nxt[j], -1)
    is_lead = leader == np.arange(n)
    slot_of = np.cumsum(is_lead) - is_lead
    lead = np.nonzero(is_lead)[0]
    lab = label[y, x]
    order = np.argsort((lab[lead] << 32) | lead, kind="stable")
    inv = np.empty(len(lead), np.int64)
    inv[order] = np.arange(len(lead))
    ring = inv[slot_of[leader]]
    nr = len(lead)
    nn = val[lead][order]
    noff = np.concatenate([[0], np.cumsum(nn)])
    N = int(noff[-1])
    pos = nn[ring] - val
    nd = np.nonzero(node)[0]
    jn = np.nonzero(node & junction)[0]
    jc = np.bincount(ring[jn], minlength=nr)
    fj = np.full(nr, 1 << 40, np.int64)
    np.minimum.at(fj, ring[jn], pos[jn])
    mc = np.full(nr, NO_TIE, np.int64)
    np.minimum.at(mc, ring[nd], (cidx[nd] << 32) | pos[nd])
    rot = np.where(jc > 0, fj, mc & 0xFFFFFFFF)
    Q = noff[ring[nd]] + (pos[nd] - rot[ring[nd]]) % nn[ring[nd]]
    A = {k_: np.zeros(N, np.int64) for k_ in ("x", "y", "c", "z", "right", "junc", "ring")}
    for k_, v in (("x", X), ("y", Y), ("c", cidx), ("z", zn), ("right", right), ("junc", junction), ("ring", ring)):
        A[k_][Q] = v[nd]
    A.update(noff=noff, nn=nn, rot=rot, jc=jc, N=N, nr=nr)
    return plain, A


def walk_cells(x0, y0, x1, y1, k):
    """the cells of every segment, column of cells by column: (segment, cx, cy) arrays in the device's order"""
    swap = x0 > x1
    x0, y0, x1, y1 = np.where(swap, x1, x0), np.where(swap, y1, y0), np.where(swap, x0, x1), np.where(swap, y0, y1)
    dx, dy = x1 - x0, y1 - y0
    ncol = (x1 >> k) - (x0 >> k) + 1
    s = np.repeat(np.arange(len(x0)), ncol)
    cx = (x0 >> k)[s] + np.arange(len(s)) - np.repeat(np.cumsum(ncol) - ncol, ncol)
    xa, xb = np.maximum(x0[s], cx << k), np.minimum(x1[s], (cx + 1) << k)
    den = np.where(dx[s] == 0, 1, dx[s])
    fa = np.where(dx[s] == 0, np.minimum(y0, y1)[s], (y0[s] * dx[s] + (xa - x0[s]) * dy[s]) // den)
    fb = np.where(dx[s] == 0, np.maximum(y0, y1)[s], (y0[s] * dx[s] + (xb - x0[s]) * dy[s]) // den)
    lo, hi = np.minimum(fa, fb) >> k, np.maximum(fa, fb) >> k
    nrow = hi - lo + 1
    t = np.repeat(np.arange(len(s)), nrow)
    cy = lo[t] + np.arange(len(t)) - np.repeat(np.cumsum(nrow) - nrow, nrow)
    return s[t], cx[t], cy


def conflicts(a, al, ar, b, bl, br):
    """a, b: (x0, y0, x1, y1) arrays of the two segments of every pair; their labels.  The pairs that conflict."""
    def orient(ux, uy, vx, vy, px, py):
        return (vx - ux) * (py - uy) - (vy - uy) * (px - ux)

    def inside_open(ux, uy, vx, vy, px, py):
        return ((px >= np.minimum(ux, vx)) & (px <= np.maximum(ux, vx)) & (py >= np.minimum(uy, vy)) & (py <= np.maximum(uy, vy)) &
                ~((px == ux) & (py == uy)) & ~((px == vx) & (py == vy)))

    twin = (a[0] == b[2]) & (a[1] == b[3]) & (a[2] == b[0]) & (a[3] == b[1]) & (al == br) & (ar == bl)
    d1, d2 = orient(b[0], b[1], b[2], b[3], a[0], a[1]), orient(b[0], b[1], b[2], b[3], a[2], a[3])
    d3, d4 = orient(a[0], a[1], a[2], a[3], b[0], b[1]), orient(a[0], a[1], a[2], a[3], b[2], b[3])
    proper = (((d1 > 0) & (d2 < 0)) | ((d1 < 0) & (d2 > 0))) & (((d3 > 0) & (d4 < 0)) | ((d3 < 0) & (d4 > 0)))
    col = (d1 == 0) & (d2 == 0) & (d3 == 0) & (d4 == 0)
    a0, a1, b0, b1 = (a[0] << 32) | a[1], (a[2] << 32) | a[3], (b[0] << 32) | b[1], (b[2] << 32) | b[3]
    overlap = col & (np.maximum(np.minimum(a0, a1), np.minimum(b0, b1)) < np.minimum(np.maximum(a0, a1), np.maximum(b0, b1)))
    touch = ~col & (((d1 == 0) & inside_open(b[0], b[1], b[2], b[3], a[0], a[1])) |
                    ((d2 == 0) & inside_open(b[0], b[1], b[2], b[3], a[2], a[3])) |
                    ((d3 == 0) & inside_open(a[0], a[1], a[2], a[3], b[0], b[1])) |
                    ((d4 == 0) & inside_open(a[0], a[1], a[2], a[3], b[2], b[3])))
    return ~twin & (proper | overlap | touch)


def clean(label, top=None, n_labels=None, num=0, den=1, max_rounds=-1, cell_log2=0, trace=None):
    """returns (the plain outlines, the simplified outlines, the clean outlines); trace: a dict that receives the most
    cells one segment touched"""
    label = np.asarray(label, np.int64)
    h, w = label.shape
    k = cell_log2 if cell_log2 else DEFAULT_CELL_LOG2
    plain, simple = sref.simplify(label, top, n_labels, num, den)
    if plain.n_half == 0:
        res = brute.sb.pack([], top is not None, 0, 0, 0, 0)
        for f in brute.TOTALS + ("n_entries", "max_cell_entries"):
            setattr(res, f, 0)
        return plain, simple, res
    _, A = node_arrays(label, top, n_labels)
    N, nr, noff, nring, nx, ny, nc = A["N"], A["nr"], A["noff"], A["ring"], A["x"], A["y"], A["c"]
    assert N == simple.n_nodes
    # the kept flags of the simplified outlines: a ring visits a corner twice only at junction nodes, which are all kept
    vring = np.repeat(np.arange(nr), simple.s_ring_vertices)
    vc = simple.sxy[:, 1].astype(np.int64) * (w + 1) + simple.sxy[:, 0]
    kept = np.isin((nring << 34) | nc, (vring << 34) | vc)
    assert kept.sum() == simple.n_svertices
    kept0 = kept.copy()
    rlabel = np.asarray(plain.ring_label, np.int64)
    ncx = (w >> k) + 1
    rounds, n_marked_first, n_entries, max_cell, max_span = 0, None, 0, 0, 0
    while True:
        # ---- detect
        kscan = np.concatenate([[0], np.cumsum(kept)])
        klist = np.nonzero(kept)[0]
        nseg = len(klist)
        j = np.arange(nseg)
        r = nring[klist]
        R = np.where(j + 1 < kscan[noff[r + 1]], klist[np.minimum(j + 1, nseg - 1)], noff[r])
        sx0, sy0, sx1, sy1 = nx[klist], ny[klist], nx[R], ny[R]
        left, right = rlabel[r], A["right"][klist]
        es, ecx, ecy = walk_cells(sx0, sy0, sx1, sy1, k)
        max_span = max(max_span, int(np.bincount(es).max()))
        key = ecy * ncx + ecx
        order = np.argsort(key, kind="stable")
        key, val = key[order], es[order]
        E = len(key)
        first = np.searchsorted(key, key, "left")
        last = np.searchsorted(key, key, "right")
        max_cell = max(max_cell, int((last - first).max()))
        c = last - np.arange(E) - 1  # partners behind every entry in its run
        i = np.repeat(np.arange(E), c)
        p = np.arange(len(i)) - np.repeat(np.cumsum(c) - c, c) + i + 1
        sa, sb_ = val[i], val[p]
        bx0, bx1, by0, by1 = np.minimum(sx0, sx1), np.maximum(sx0, sx1), np.minimum(sy0, sy1), np.maximum(sy0, sy1)
        near = (bx1[sa] >= bx0[sb_]) & (bx1[sb_] >= bx0[sa]) & (by1[sa] >= by0[sb_]) & (by1[sb_] >= by0[sa])
        sa, sb_ = sa[near], sb_[near]  # (the device's first reject: boxes that are apart)
        hit = conflicts((sx0[sa], sy0[sa], sx1[sa], sy1[sa]), left[sa], right[sa], (sx0[sb_], sy0[sb_], sx1[sb_], sy1[sb_]),
                        left[sb_], right[sb_])
        mark = np.zeros(nseg, bool)
        mark[sa[hit]] = True
        mark[sb_[hit]] = True
        n_marked = int(mark.sum())
        if n_marked_first is None:
            n_marked_first, n_entries = n_marked, E
        if n_marked == 0 or rounds == max_rounds:
            break
        assert rounds < N
        # ---- repair: the dropped nodes of marked segments, their segment (L, R), the greatest c^2, the lowest corner
        q = np.nonzero(~kept)[0]
        q = q[mark[kscan[q] - 1]]
        sj = kscan[q] - 1
        Ln, Rn = klist[sj], R[sj]
        cr = (nx[Rn] - nx[Ln]) * (ny[q] - ny[Ln]) - (ny[Rn] - ny[Ln]) * (nx[q] - nx[Ln])
        m = cr * cr
        best = np.zeros(N, np.int64)
        np.maximum.at(best, Ln, m)
        tie = np.full(N, NO_TIE, np.int64)
        top_ = (m == best[Ln]) & (m > 0)
        np.minimum.at(tie, Ln[top_], (nc[q[top_]] << 32) | q[top_])
        picks = tie[tie != NO_TIE] & 0xFFFFFFFF
        kept = kept.copy()
        kept[picks] = True
        rounds += 1
    # ---- rings: the un-rotation of the kept nodes, flags, area2
    nn, rot, jc = A["nn"], A["rot"], A["jc"]
    soff = kscan[noff]
    kcount = np.diff(soff)
    kq = klist
    rk = nring[kq]
    kb = kscan[noff[rk] + nn[rk] - rot[rk]] - soff[rk]
    dest = soff[rk] + (kscan[kq] - soff[rk] - kb) % kcount[rk]
    nsv = int(soff[-1])
    assert np.array_equal(np.sort(dest), np.arange(nsv))
    sxy = np.zeros((nsv, 2), np.int32)
    sz, s_right, s_flag = np.zeros(nsv, np.int32), np.zeros(nsv, np.int32), np.zeros(nsv, np.uint8)
    sxy[dest, 0], sxy[dest, 1], sz[dest], s_right[dest] = nx[kq], ny[kq], A["z"][kq], A["right"][kq]
    lone = (kq == noff[rk]) & (jc[rk] == 0)
    s_flag[dest] = A["junc"][kq] | (2 * lone) | (brute.F_REPAIRED * ~kept0[kq]) | (brute.F_MARKED * mark)
    ringv = np.repeat(np.arange(nr), kcount)
    nxtv = np.where(np.arange(nsv) + 1 < soff[ringv + 1], np.arange(nsv) + 1, soff[ringv])
    area2 = np.zeros(nr, np.int64)
    sx64, sy64 = sxy[:, 0].astype(np.int64), sxy[:, 1].astype(np.int64)
    np.add.at(area2, ringv, sx64 * sy64[nxtv] - sx64[nxtv] * sy64)
    if trace is not None:
        trace["max_span"] = max_span
    from types import SimpleNamespace
    return plain, simple, SimpleNamespace(
        n_rings=nr, n_nodes=N, n_junction_nodes=simple.n_junction_nodes, n_arcs=simple.n_arcs, n_svertices=nsv,
        rounds=simple.rounds, max_arc_nodes=simple.max_arc_nodes, s_ring_vertices=kcount.astype(np.int64), s_ring_area2=area2,
        s_ring_arcs=simple.s_ring_arcs, s_ring_offset=soff.astype(np.int64), sxy=sxy, sz=sz if top is not None else None,
        s_right=s_right, s_flag=s_flag, n_svertices_before=int(simple.n_svertices), n_marked_first=n_marked_first,
        n_marked_left=n_marked, n_forced=nsv - int(simple.n_svertices), repair_rounds=rounds, n_entries=n_entries,
        max_cell_entries=max_cell)


def same(a, b, fields=brute.FIELDS):
    """None if the two results are equal, else the name of the first field that differs"""
    for f in fields:
        u, v = getattr(a, f), getattr(b, f)
        if (u is None) != (v is None):
            return f
        if u is None:
            continue
        u, v = np.asarray(u), np.asarray(v)
        if u.shape != v.shape or not np.array_equal(u.astype(np.int64), v.astype(np.int64)):
            return f
    return None
