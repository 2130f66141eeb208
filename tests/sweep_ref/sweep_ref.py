"""Clean outlines with sweeps (include/bs_api.h, "clean outlines", paragraph "Sweeps") as the device computes them, restated
in numpy on top of the arrays of tests/uncross_ref/uncross_ref.py: `clean` of that file restated (imported, not modified) with
the sweep pass of bs_sweep.hip in every detection --
  bitmap   the kept corners
  runs     per node its segment, the ray axis by the chord's dominant direction (coordinates swapped where |dx| < |dy|: the
           rays are vertical in the swapped frame), and one item per lattice line that the run to the next node crosses
  items    the corners of the line between the run and the chord's crossing (floor and ceiling), or the nearer chord end
  test     candidates that are a kept corner and no end of the segment are hits; every hit is tested exactly: boundary,
           signed crossings of the upward ray, and the first run of the line whose interval holds the corner
  marks    sweeping, sweeping-only; OR-ed into the conflict marks in mode 2
with the layout's own figures.  tests/sweep_ref/brute.py tests every position against every lens; the two must be equal."""
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
brute = _load("sweep_brute", os.path.join(HERE, "brute.py"))
sref, ubrute = uref.sref, uref.brute

WAVE_CAP = 64  # BS_SWEEP_WAVE_CAP
GRID_STRIDE = 1024 * 256  # the threads of one sweep of a grid-stride pass
LAYOUT_TOTALS = ("n_items_first", "n_items_swapped_first", "n_candidates_first", "n_exact_first", "n_exact_wave_first",
                 "n_rejected_first")
SWEEP_FIELDS = brute.SWEEP_TOTALS + LAYOUT_TOTALS
DEVICE_FIELDS = uref.DEVICE_FIELDS  # of the clean result
NO_TIE = uref.NO_TIE


def chord_ref(ax, ay, bx, by, X):
    """floor and ceiling of the chord's Y on the line X where it crosses it (half-open), else the Y of the nearer end"""
    mn, mx = np.minimum(ax, bx), np.maximum(ax, bx)
    cross = (X >= mn) & (X < mx)
    dx = np.where(cross, bx - ax, 1)
    num = (X - ax) * (by - ay)
    flo_c = ay + np.floor_divide(num, dx)
    cei_c = ay - np.floor_divide(-num, dx)
    end = np.where((X < mn) == (ax <= bx), ay, by)
    return np.where(cross, flo_c, end), np.where(cross, cei_c, end)


def detect(A, w, kept, kscan, klist, Rj, mark):
    """one detection's sweep pass: (smark [nseg] bool, figures of the detection)"""
    N, noff, nring, nx, ny = A["N"], A["noff"], A["ring"], A["x"], A["y"]
    q = np.arange(N)
    r0, r1 = noff[nring], noff[nring + 1]
    j = np.where(kept, kscan[:N], kscan[:N] - 1)
    L, R = klist[j], Rj[j]
    lens = (R != L) & (np.where(L + 1 < r1, L + 1, r0) != R)
    T = np.abs(nx[R] - nx[L]) < np.abs(ny[R] - ny[L])

    def tr(x, y):
        return np.where(T, y, x), np.where(T, x, y)

    ax, ay = tr(nx[L], ny[L])
    bx, by = tr(nx[R], ny[R])
    nq = np.where(q + 1 < r1, q + 1, r0)
    px, py = tr(nx, ny)
    qx, qy = tr(nx[nq], ny[nq])
    icnt = np.where(lens & (py == qy), np.abs(qx - px), 0)
    fig = dict(n_lens=int((lens & (q == L)).sum()), n_items=int(icnt.sum()), n_items_swapped=int(icnt[T].sum()), n_candidates=0,
               n_exact=0, n_exact_wave=0, n_rejected=0, n_pairs=0, max_w=0)
    nseg = len(klist)
    smark = np.zeros(nseg, bool)
    if fig["n_items"]:
        node = np.repeat(q, icnt)
        X = np.minimum(px, qx)[node] + np.arange(len(node)) - np.repeat(np.cumsum(icnt) - icnt, icnt)
        flo, cei = chord_ref(ax[node], ay[node], bx[node], by[node], X)
        lo, hi = np.minimum(py[node], flo), np.maximum(py[node], cei)
        ccnt = hi - lo + 1
        fig["n_candidates"] = int(ccnt.sum())
        it = np.repeat(np.arange(len(node)), ccnt)
        cy = lo[it] + np.arange(len(it)) - np.repeat(np.cumsum(ccnt) - ccnt, ccnt)
        cx, cq = X[it], node[it]
        realx, realy = np.where(T[cq], cy, cx), np.where(T[cq], cx, cy)
        corners = np.unique(ny[kept] * (w + 1) + nx[kept])  # the bitmap
        hit = np.isin(realy * (w + 1) + realx, corners)
        hit &= ~((cx == ax[cq]) & (cy == ay[cq])) & ~((cx == bx[cq]) & (cy == by[cq]))
        seen = set()
        for c in np.flatnonzero(hit):  # the exact tests
            n0 = int(cq[c])
            l0, rr0, rr1 = int(L[n0]), int(r0[n0]), int(r1[n0])
            cnt = (int(R[n0]) - l0) % (rr1 - rr0) or (rr1 - rr0)
            fig["n_exact"] += 1
            fig["n_exact_wave"] += cnt > WAVE_CAP
            e = np.arange(cnt)
            qi = rr0 + (l0 - rr0 + e) % (rr1 - rr0)
            qn = np.where(qi + 1 < rr1, qi + 1, rr0)
            t = bool(T[n0])
            ex, ey = (ny[qi], nx[qi]) if t else (nx[qi], ny[qi])
            fx, fy = (ny[qn], nx[qn]) if t else (nx[qn], ny[qn])
            wx, wy = int(cx[c]), int(cy[c])
            a, b = (int(ax[n0]), int(ay[n0])), (int(bx[n0]), int(by[n0]))
            vert, hor = ex == fx, ey == fy
            mn, mx = np.minimum(ex, fx), np.maximum(ex, fx)
            onb = bool((vert & (wx == ex) & (wy >= np.minimum(ey, fy)) & (wy <= np.maximum(ey, fy))).any() or
                       (hor & ~vert & (wy == ey) & (wx >= mn) & (wx <= mx)).any())
            on_line = hor & ~vert & (wx >= mn) & (wx < mx)
            wn = int(np.where(on_line & (ey > wy), np.where(ex < fx, 1, -1), 0).sum())
            f0, c0 = (int(v) for v in chord_ref(*(np.int64(v) for v in a + b), np.int64(wx)))
            holds = on_line & (wy >= np.minimum(ey, f0)) & (wy <= np.maximum(ey, c0))
            first = int(np.flatnonzero(holds)[0])
            o = brute.orient(b, a, (wx, wy))  # the chord runs b -> a
            if o == 0 and min(a[0], b[0]) <= wx <= max(a[0], b[0]) and min(a[1], b[1]) <= wy <= max(a[1], b[1]):
                onb = True
            if min(a[0], b[0]) <= wx < max(a[0], b[0]):
                wn += 1 if (b[0] < a[0] and o < 0) else (-1 if (b[0] > a[0] and o > 0) else 0)
            if onb or wn == 0:
                fig["n_rejected"] += 1
                continue
            smark[j[n0]] = True
            fig["max_w"] = max(fig["max_w"], abs(wn))
            if first == n0 - l0:
                fig["n_pairs"] += 1
                key = (int(realx[c]), int(realy[c]), int(j[n0]))
                assert key not in seen  # (a pair is counted by one item only)
                seen.add(key)
    fig["n_sweeping"] = int(smark.sum())
    fig["n_only"] = int((smark & ~mark).sum())
    return smark, fig


def clean(label, top=None, n_labels=None, num=0, den=1, max_rounds=-1, cell_log2=0, mode=2, trace=None):
    """returns (the plain outlines, the simplified outlines, the clean outlines with the sweep figures as attributes)"""
    label = np.asarray(label, np.int64)
    h, w = label.shape
    k = cell_log2 if cell_log2 else uref.DEFAULT_CELL_LOG2
    plain, simple = sref.simplify(label, top, n_labels, num, den)
    zero = dict(mode=mode, **{f: 0 for f in SWEEP_FIELDS})
    if plain.n_half == 0:
        res = ubrute.sb.pack([], top is not None, 0, 0, 0, 0)
        for f in ubrute.TOTALS + ("n_entries", "max_cell_entries"):
            setattr(res, f, 0)
        res.__dict__.update(zero)
        return plain, simple, res
    _, A = uref.node_arrays(label, top, n_labels)
    N, nr, noff, nring, nx, ny, nc = A["N"], A["nr"], A["noff"], A["ring"], A["x"], A["y"], A["c"]
    vring = np.repeat(np.arange(nr), simple.s_ring_vertices)
    vc = simple.sxy[:, 1].astype(np.int64) * (w + 1) + simple.sxy[:, 0]
    kept = np.isin((nring << 34) | nc, (vring << 34) | vc)
    assert kept.sum() == simple.n_svertices
    kept0 = kept.copy()
    rlabel = np.asarray(plain.ring_label, np.int64)
    ncx = (w >> k) + 1
    rounds, n_marked_first, n_entries, max_cell = 0, None, 0, 0
    first_fig, max_w, sweep_rounds, figs = None, 0, 0, []
    while True:
        # ---- detect (tests/uncross_ref/uncross_ref.py)
        kscan = np.concatenate([[0], np.cumsum(kept)])
        klist = np.nonzero(kept)[0]
        nseg = len(klist)
        j = np.arange(nseg)
        r = nring[klist]
        R = np.where(j + 1 < kscan[noff[r + 1]], klist[np.minimum(j + 1, nseg - 1)], noff[r])
        sx0, sy0, sx1, sy1 = nx[klist], ny[klist], nx[R], ny[R]
        left, right = rlabel[r], A["right"][klist]
        es, ecx, ecy = uref.walk_cells(sx0, sy0, sx1, sy1, k)
        key = ecy * ncx + ecx
        order = np.argsort(key, kind="stable")
        key, val = key[order], es[order]
        E = len(key)
        first = np.searchsorted(key, key, "left")
        last = np.searchsorted(key, key, "right")
        max_cell = max(max_cell, int((last - first).max()))
        c = last - np.arange(E) - 1
        i = np.repeat(np.arange(E), c)
        p = np.arange(len(i)) - np.repeat(np.cumsum(c) - c, c) + i + 1
        sa, sb_ = val[i], val[p]
        bx0, bx1, by0, by1 = np.minimum(sx0, sx1), np.maximum(sx0, sx1), np.minimum(sy0, sy1), np.maximum(sy0, sy1)
        near = (bx1[sa] >= bx0[sb_]) & (bx1[sb_] >= bx0[sa]) & (by1[sa] >= by0[sb_]) & (by1[sb_] >= by0[sa])
        sa, sb_ = sa[near], sb_[near]
        hit = uref.conflicts((sx0[sa], sy0[sa], sx1[sa], sy1[sa]), left[sa], right[sa], (sx0[sb_], sy0[sb_], sx1[sb_], sy1[sb_]),
                             left[sb_], right[sb_])
        mark = np.zeros(nseg, bool)
        mark[sa[hit]] = True
        mark[sb_[hit]] = True
        # ---- the sweep pass
        smark = np.zeros(nseg, bool)
        if mode:
            smark, fig = detect(A, w, kept, kscan, klist, R, mark)
            figs.append(fig)
            if first_fig is None:
                first_fig = fig
            max_w = max(max_w, fig["max_w"])
        n_marked = int(mark.sum())  # (conflicts only)
        todo = mark | smark if mode == 2 else mark
        if n_marked_first is None:
            n_marked_first, n_entries = n_marked, E
        if not todo.any() or rounds == max_rounds:
            break
        assert rounds < N
        if mode == 2 and smark.any():
            sweep_rounds += 1
        # ---- repair (tests/uncross_ref/uncross_ref.py, over the union of the marks)
        q = np.nonzero(~kept)[0]
        q = q[todo[kscan[q] - 1]]
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
    # ---- rings
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
    s_flag[dest] = (A["junc"][kq] | (2 * lone) | (brute.F_REPAIRED * ~kept0[kq]) | (brute.F_MARKED * mark) |
                    (brute.F_SWEEPING * smark))
    ringv = np.repeat(np.arange(nr), kcount)
    nxtv = np.where(np.arange(nsv) + 1 < soff[ringv + 1], np.arange(nsv) + 1, soff[ringv])
    area2 = np.zeros(nr, np.int64)
    sx64, sy64 = sxy[:, 0].astype(np.int64), sxy[:, 1].astype(np.int64)
    np.add.at(area2, ringv, sx64 * sy64[nxtv] - sx64[nxtv] * sy64)
    if trace is not None:
        trace["detections"] = figs
    res = SimpleNamespace(
        n_rings=nr, n_nodes=N, n_junction_nodes=simple.n_junction_nodes, n_arcs=simple.n_arcs, n_svertices=nsv,
        rounds=simple.rounds, max_arc_nodes=simple.max_arc_nodes, s_ring_vertices=kcount.astype(np.int64), s_ring_area2=area2,
        s_ring_arcs=simple.s_ring_arcs, s_ring_offset=soff.astype(np.int64), sxy=sxy, sz=sz if top is not None else None,
        s_right=s_right, s_flag=s_flag, n_svertices_before=int(simple.n_svertices), n_marked_first=n_marked_first,
        n_marked_left=n_marked, n_forced=nsv - int(simple.n_svertices), repair_rounds=rounds, n_entries=n_entries,
        max_cell_entries=max_cell, **zero)
    if mode:
        f = first_fig
        res.__dict__.update(
            n_lens_segments_first=f["n_lens"], n_sweeping_first=f["n_sweeping"], n_sweeping_only_first=f["n_only"],
            n_swept_pairs_first=f["n_pairs"], max_abs_winding=max_w, sweep_rounds=sweep_rounds, n_sweeping_left=int(smark.sum()),
            n_items_first=f["n_items"], n_items_swapped_first=f["n_items_swapped"], n_candidates_first=f["n_candidates"],
            n_exact_first=f["n_exact"], n_exact_wave_first=f["n_exact_wave"], n_rejected_first=f["n_rejected"])
    return plain, simple, res


def same(a, b, fields):
    """None if the two results are equal in the fields, else the name of the first field that differs"""
    return uref.same(a, b, fields)
