"""Simplified outlines (include/bs_api.h, "simplified outlines") as the device computes them, restated in numpy: the
junction test and node flag per compact half-edge, R Wyllie rounds that carry node counts, the per-ring junction count,
first junction node and lowest corner, the rotation, arc ids from a scan, the closed pass that keeps F, then synchronous
rounds -- per segment (named by the kept node at its left end) the greatest c^2, then the lowest (corner, place) among
the nodes that reach it, then the decision -- until a round keeps nothing, and the un-rotation of the kept nodes.
tests/simplify_ref/brute.py recurses per arc instead; the two must be equal, `rounds` included."""
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


orf = _load("outline_ref", os.path.join(HERE, "..", "outline_ref", "outline_ref.py"))
brute = _load("simplify_brute", os.path.join(HERE, "brute.py"))

END = -1
KEPT, DROPPED = -1, -2  # seg[:, 0] of a node that is no longer active
NO_TIE = (1 << 63) - 1


def empty(has_z):
    return brute.pack([], has_z, 0, 0, 0, 0)


def simplify(label, top=None, n_labels=None, num=0, den=1, trace=None):
    """returns (the plain outlines, the simplified outlines); trace: a dict that receives what the regime test reads"""
    label = np.asarray(label, np.int64)
    h, w = label.shape
    tr = {}
    plain = orf.outlines(label, top, n_labels, trace=tr)
    stats = dict(closed_arcs=0, one_junction_rings=0, saddles=0, junction_not_vertex=0, ties=0, forced_only=0,
                 max_product=0, empty_arcs=0)
    if trace is not None:
        trace.update(stats)
    if plain.n_half == 0:
        return plain, empty(top is not None)
    succ, vert, leader, hnum, R = tr["succ"], tr["vert"], tr["leader"], tr["hnum"], tr["R"]
    n = len(hnum)
    # ---- nodes: the junction test of the start corner, node flag, right label, corner index, Z
    p, k = hnum >> 2, hnum & 3
    x, y = p % w, p // w
    X, Y = x + orf.SX[k], y + orf.SY[k]
    L = np.pad(np.maximum(label, -1), 1, constant_values=-1)  # L[y + 1, x + 1]
    a, b, c, d = L[Y, X], L[Y, X + 1], L[Y + 1, X], L[Y + 1, X + 1]
    distinct = 1 + (b != a) + ((c != a) & (c != b)) + ((d != a) & (d != b) & (d != c))
    saddle = (a == d) & (b == c) & (a != b)
    junction = (distinct >= 3) | saddle
    node = vert | junction
    right = L[y + orf.DY[k] + 1, x + orf.DX[k] + 1]
    cidx = Y * (w + 1) + X
    zn = np.asarray(top)[y, x, orf.ZIDX[k]] if top is not None else np.zeros(n, np.int64)
    stats["saddles"] = int(saddle.sum())
    stats["junction_not_vertex"] = int((junction & ~vert).sum())
    # ---- placing: the cut in front of the leader, R Wyllie rounds that carry node counts
    nxt = np.where(succ == leader, END, succ)
    val = node.astype(np.int64)
    for _ in range(R):
        live = nxt != END
        j = np.where(live, nxt, 0)
        val, nxt = np.where(live, val + val[j], val), np.where(live, nxt[j], END)
    assert (nxt == END).all()
    is_lead = leader == np.arange(n)
    slot_of = np.cumsum(is_lead) - is_lead
    lead = np.nonzero(is_lead)[0]
    lab = label[y, x]
    order = np.argsort((lab[lead] << 32) | lead, kind="stable")
    inv = np.empty(len(lead), np.int64)
    inv[order] = np.arange(len(lead))
    ring = inv[slot_of[leader]]
    nr = len(lead)
    nn = val[lead][order]  # nodes per ring
    noff = np.concatenate([[0], np.cumsum(nn)])
    N = int(noff[-1])
    pos = nn[ring] - val  # place in walk order from h0 (of nodes)
    # ---- arcs: junction count, first junction node, lowest corner per ring; the rotation
    nd = np.nonzero(node)[0]
    jn = np.nonzero(node & junction)[0]
    jc = np.bincount(ring[jn], minlength=nr)
    fj = np.full(nr, 1 << 40, np.int64)
    np.minimum.at(fj, ring[jn], pos[jn])
    mc = np.full(nr, NO_TIE, np.int64)
    np.minimum.at(mc, ring[nd], (cidx[nd] << 32) | pos[nd])
    rot = np.where(jc > 0, fj, mc & 0xFFFFFFFF)
    stats["one_junction_rings"] = int((jc == 1).sum())
    Q = noff[ring[nd]] + (pos[nd] - rot[ring[nd]]) % nn[ring[nd]]
    assert np.array_equal(np.sort(Q), np.arange(N))
    nx, ny, nc, nz, nright, njunc, nring = (np.zeros(N, np.int64) for _ in range(7))
    nx[Q], ny[Q], nc[Q], nz[Q], nright[Q], njunc[Q], nring[Q] = X[nd], Y[nd], cidx[nd], zn[nd], right[nd], junction[nd], ring[nd]
    idx = np.arange(N)
    first = idx == noff[nring]
    start = (njunc == 1) | first
    arc = np.cumsum(start) - 1
    astart = np.nonzero(start)[0]
    n_arcs = len(astart)
    # the segment of every node: (left kept node, right kept node); the last arc of a ring ends at the ring's first node
    nxt_start = np.where(arc + 1 < n_arcs, astart[np.minimum(arc + 1, n_arcs - 1)], N)
    ring_end = noff[nring + 1]
    seg = np.stack([np.where(start, KEPT, astart[arc]), np.where(nxt_start < ring_end, nxt_start, noff[nring])], 1)
    arc_nodes = np.minimum(nxt_start, ring_end)[astart] - astart + 1
    stats["empty_arcs"] = int((arc_nodes == 2).sum())

    def one_round(seg, closed, forced):
        """one pass over all nodes: returns (the next seg, the next forced or None, whether a node was kept)"""
        act = np.nonzero(seg[:, 0] >= 0)[0]
        l, r = seg[act, 0], seg[act, 1]
        if closed:  # only the nodes of closed arcs take part, and the measure is the squared distance from the start
            take = nc[l] == nc[r]
            act, l, r = act[take], l[take], r[take]
            m = (nx[act] - nx[l]) ** 2 + (ny[act] - ny[l]) ** 2
        else:
            cr = (nx[r] - nx[l]) * (ny[act] - ny[l]) - (ny[r] - ny[l]) * (nx[act] - nx[l])
            m = cr * cr
        best = np.zeros(N, np.int64)
        np.maximum.at(best, l, m)
        tie = np.full(N, NO_TIE, np.int64)
        top_ = m == best[l]
        np.minimum.at(tie, l[top_], (nc[act[top_]] << 32) | act[top_])
        heads = np.unique(l)
        stats["ties"] += int((np.bincount(l[top_], minlength=N)[heads] > 1).sum())
        len2 = (nx[r] - nx[l]) ** 2 + (ny[r] - ny[l]) ** 2
        b = best[l]
        beyond = np.zeros(len(act), bool)
        ev = np.zeros(len(act), bool) if closed else (forced[l] != 1 if forced is not None else np.ones(len(act), bool))
        if ev.any():  # (the comparison is evaluated only where it decides)
            big = max(int(b[ev].max()) * den, num * int(len2[ev].max()))
            stats["max_product"] = max(stats["max_product"], big)
            if big < 1 << 63:
                beyond[ev] = b[ev] * den > num * len2[ev]
            else:  # Python integers where a product passes 63 bits
                beyond[ev] = np.array([int(u) * den > num * int(v) for u, v in zip(b[ev], len2[ev])], bool)
        if closed:
            split = np.ones(len(act), bool)
        elif forced is not None:
            split = np.where(forced[l] == 1, b > 0, beyond)
            fo = (forced[l] == 1) & (b > 0)  # forced splits that the tolerance alone would not make
            if fo.any():
                stats["forced_only"] += int(len(np.unique(l[fo][[int(u) * den <= num * int(v) for u, v in zip(b[fo], len2[fo])]])))
        else:
            split = beyond
        pick = tie[l] & 0xFFFFFFFF
        out = seg.copy()
        out[act[~split], 0] = DROPPED
        s = split & (pick == act)
        out[act[s], 0] = KEPT
        lo, hi = split & (act < pick), split & (act > pick)
        out[act[lo], 1] = pick[lo]
        out[act[hi], 0] = pick[hi]
        nf = None
        if closed:
            nf = np.zeros(N, np.int64)
            nf[l[s]] = 1
            nf[act[s]] = 1
        return out, nf, bool(s.any())

    closed_arc = nc[astart] == nc[np.where(nxt_start < ring_end, nxt_start, noff[nring])[astart]]
    stats["closed_arcs"] = int(closed_arc.sum())
    seg, forced, _ = one_round(seg, True, None)
    forced = np.maximum(forced, start.astype(np.int64))  # the first split of every arc is forced, open arcs included
    rounds = 0
    while True:
        seg, _, any_kept = one_round(seg, False, forced)
        forced = None
        if not any_kept:
            break
        rounds += 1
    assert (seg[:, 0] < 0).all()
    # ---- rings: kept counts by a scan, the un-rotation, area2
    kept = seg[:, 0] == KEPT
    kscan = np.concatenate([[0], np.cumsum(kept)])
    soff = kscan[noff]
    kcount = np.diff(soff)
    kq = np.nonzero(kept)[0]
    rk = nring[kq]
    kb = kscan[noff[rk] + nn[rk] - rot[rk]] - soff[rk]  # kept nodes of the ring in front of h0's place in the rotated order
    dest = soff[rk] + (kscan[kq] - soff[rk] - kb) % kcount[rk]
    nsv = int(soff[-1])
    assert np.array_equal(np.sort(dest), np.arange(nsv))
    sxy = np.zeros((nsv, 2), np.int32)
    sz, s_right, s_flag = np.zeros(nsv, np.int32), np.zeros(nsv, np.int32), np.zeros(nsv, np.uint8)
    sxy[dest, 0], sxy[dest, 1], sz[dest], s_right[dest] = nx[kq], ny[kq], nz[kq], nright[kq]
    s_flag[dest] = njunc[kq] | (2 * (first[kq] & (jc[rk] == 0)))
    ringv = np.repeat(np.arange(nr), kcount)
    nxtv = np.where(np.arange(nsv) + 1 < soff[ringv + 1], np.arange(nsv) + 1, soff[ringv])
    area2 = np.zeros(nr, np.int64)
    sx64, sy64 = sxy[:, 0].astype(np.int64), sxy[:, 1].astype(np.int64)
    np.add.at(area2, ringv, sx64 * sy64[nxtv] - sx64[nxtv] * sy64)
    if trace is not None:
        trace.update(stats)
    return plain, SimpleNamespace(
        n_rings=nr, n_nodes=N, n_junction_nodes=int(njunc.sum()), n_arcs=n_arcs, n_svertices=nsv, rounds=rounds,
        max_arc_nodes=int(arc_nodes.max()), s_ring_vertices=kcount.astype(np.int64), s_ring_area2=area2,
        s_ring_arcs=np.maximum(jc, 1).astype(np.int64), s_ring_offset=soff.astype(np.int64), sxy=sxy,
        sz=sz if top is not None else None, s_right=s_right, s_flag=s_flag)


def same(a, b):
    """None if the two results are equal, else the name of the first field that differs"""
    for f in brute.FIELDS:
        u, v = getattr(a, f), getattr(b, f)
        if (u is None) != (v is None):
            return f
        if u is None:
            continue
        u, v = np.asarray(u), np.asarray(v)
        if u.shape != v.shape or not np.array_equal(u.astype(np.int64), v.astype(np.int64)):
            return f
    return None
