"""CPU restatement of the roof stage (include/bs_api.h, "roofs") that the roof tests compare the device against.
numpy, in another formulation than the device's: np.unique + lexsort for the vote (no sort of 64-bit keys with run
lengths, no atomics), whole-array shifted-neighbour rounds for the fill (no worklists), bincount / reduceat for the
figures, and the OBJ text line by line."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
FIGURES = ("pixels", "seed_pixels", "bbox", "n_support", "z_min", "z_max", "z_sum")
TOTALS = ("fill_rounds", "seeded_pixels", "filled_pixels", "unroofed_pixels")


def homes(normal, plane_building, votes_in, votes_total, min_normal_z=0.5):
    """home int32 [n_planes]: the building a plane may be a roof in, or -1."""
    nz = np.asarray(normal, np.float64).reshape(-1, 3)[:, 2]
    pb = np.asarray(plane_building, np.int64)
    with np.errstate(invalid="ignore"):
        ok = (nz >= min_normal_z) & (pb >= 0) & (2 * np.asarray(votes_in, np.int64) > np.asarray(votes_total, np.int64))
    return np.where(ok, pb, -1).astype(np.int32)


def counting(xyz, bmap, plane_idx, n_planes, home, bin, ground_th):
    """(counts bool [n], pixel int64 [n]); raises IndexError if a pixel lies outside the image."""
    xyz = np.asarray(xyz, np.int64)
    h, w = bmap.shape
    if (xyz[:, :2] < 0).any():
        raise IndexError("negative coordinate")
    px, py = xyz[:, 0] // bin, xyz[:, 1] // bin
    if (px >= w).any() or (py >= h).any():
        raise IndexError("pixel outside the image")
    pix = py * w + px
    p = np.asarray(plane_idx, np.int64)
    ok = ~(xyz[:, 2].astype(np.float64) < ground_th) & (p >= 1) & (p <= n_planes)
    b = bmap.ravel()[pix]
    hm = np.full(len(p), -1, np.int64)
    if n_planes:
        hm[ok] = np.asarray(home, np.int64)[p[ok] - 1]
    ok &= (b >= 0) & (hm == b)
    return ok, pix


def vote(ok, pix, plane_idx, bmap, n_planes, min_votes):
    """(roof, support) int32 [h][w] of the vote alone."""
    h, w = bmap.shape
    roof = np.where(bmap.ravel() < 0, -1, 0).astype(np.int32)
    support = np.zeros(h * w, np.int32)
    if ok.any():
        pair, cnt = np.unique(pix[ok] * (n_planes + 1) + np.asarray(plane_idx, np.int64)[ok], return_counts=True)
        ppix, pplane = np.divmod(pair, n_planes + 1)
        order = np.lexsort((pplane, -cnt, ppix))  # by pixel, then the larger count, then the lower plane id
        upix, first = np.unique(ppix[order], return_index=True)
        win, wcnt = pplane[order[first]], cnt[order[first]]
        keep = wcnt >= min_votes
        roof[upix[keep]] = win[keep]
        support[upix[keep]] = wcnt[keep]
    return roof.reshape(h, w), support.reshape(h, w)


def _shift(a, dy, dx, fill):
    """a moved so that out[y][x] = a[y + dy][x + dx], `fill` outside the image"""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def fill_round(roof, bmap):
    """One synchronous round: (roof after it, the pixels it changed)."""
    cand = np.full(roof.shape, I32_MAX, np.int32)
    for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
        nr, nm = _shift(roof, dy, dx, 0), _shift(bmap, dy, dx, -2)
        np.minimum(cand, np.where((nm == bmap) & (nr > 0), nr, np.int32(I32_MAX)), out=cand)
    upd = (roof == 0) & (cand < I32_MAX)
    return np.where(upd, cand, roof), upd


def fill(roof, bmap):
    """(roof after all rounds, the number of rounds that changed something)."""
    rounds = 0
    while True:
        roof, upd = fill_round(roof, bmap)
        if not upd.any():
            return roof, rounds
        rounds += 1


def height_of(p, X, Y, normal, center, z_min, z_max):
    """H(p, X, Y) of include/bs_api.h for arrays (or scalars) of plane ids p >= 1 and integer millimetres X, Y."""
    s = np.asarray(p, np.int64) - 1
    n, c = np.asarray(normal, np.float64).reshape(-1, 3)[s], np.asarray(center, np.int64).reshape(-1, 3)[s]
    with np.errstate(all="ignore"):
        a = n[..., 0] * (np.asarray(X, np.int64).astype(np.float64) - c[..., 0].astype(np.float64))
        b = n[..., 1] * (np.asarray(Y, np.int64).astype(np.float64) - c[..., 1].astype(np.float64))
        z = c[..., 2].astype(np.float64) - (a + b) / n[..., 2]
        lo, hi = np.asarray(z_min, np.int64)[s].astype(np.float64), np.asarray(z_max, np.int64)[s].astype(np.float64)
        z = np.where(~(z >= lo), lo, z)
        z = np.where(z > hi, hi, z)
    return z.astype(np.int64)  # (finite after the clamps; the cast truncates towards zero)


def figures(ok, pix, xyz, plane_idx, roof, support, n_planes):
    n = n_planes
    out = SimpleNamespace()
    r = roof.ravel()
    sup = ok & (np.asarray(plane_idx, np.int64) == r[pix])
    s = np.asarray(plane_idx, np.int64)[sup] - 1
    z = np.asarray(xyz, np.int64)[sup, 2]
    out.n_support = np.bincount(s, minlength=n).astype(np.int64)[:n]
    out.z_min, out.z_max, out.z_sum = np.full(n, I32_MAX, np.int32), np.full(n, I32_MIN, np.int32), np.zeros(n, np.int64)
    if len(s):
        o = np.argsort(s, kind="stable")
        present, first = np.unique(s[o], return_index=True)
        out.z_min[present] = np.minimum.reduceat(z[o], first)
        out.z_max[present] = np.maximum.reduceat(z[o], first)
        out.z_sum[present] = np.add.reduceat(z[o], first)
    ys, xs = np.nonzero(roof > 0)
    q = roof[ys, xs].astype(np.int64) - 1
    out.pixels = np.bincount(q, minlength=n).astype(np.int64)[:n]
    out.seed_pixels = np.bincount(q[support[ys, xs] > 0], minlength=n).astype(np.int64)[:n]
    out.bbox = np.tile(np.array([I32_MAX, I32_MAX, I32_MIN, I32_MIN], np.int32), (n, 1))
    if len(q):
        o = np.argsort(q, kind="stable")
        present, first = np.unique(q[o], return_index=True)
        out.bbox[present, 0] = np.minimum.reduceat(xs[o], first)
        out.bbox[present, 1] = np.minimum.reduceat(ys[o], first)
        out.bbox[present, 2] = np.maximum.reduceat(xs[o], first)
        out.bbox[present, 3] = np.maximum.reduceat(ys[o], first)
    return out


def roofs(xyz, bmap, plane_idx, n_planes, home, normal, center, bin=100, ground_th=0.0, min_votes=1):
    """Everything bs_roofs computes: roof, support, height, the per-plane figures, the totals, and (for the coverage
    tests) seed_roof = the roof of the vote alone."""
    bmap = np.asarray(bmap, np.int32)
    ok, pix = counting(xyz, bmap, plane_idx, n_planes, home, bin, ground_th)
    seed_roof, support = vote(ok, pix, plane_idx, bmap, n_planes, min_votes)
    roof, rounds = fill(seed_roof, bmap)
    out = figures(ok, pix, xyz, plane_idx, roof, support, n_planes)
    out.roof, out.support, out.seed_roof, out.fill_rounds, out.n_planes = roof, support, seed_roof, rounds, n_planes
    out.counting, out.pixel = ok, pix
    out.seeded_pixels = int((support > 0).sum())
    out.filled_pixels = int((roof > 0).sum()) - out.seeded_pixels
    out.unroofed_pixels = int((roof == 0).sum())
    h, w = bmap.shape
    out.height = np.full((h, w), I32_MIN, np.int32)
    ys, xs = np.nonzero(roof > 0)
    if len(ys):
        out.height[ys, xs] = height_of(roof[ys, xs], xs.astype(np.int64) * bin + bin // 2, ys.astype(np.int64) * bin + bin // 2,
                                       normal, center, out.z_min, out.z_max)
    return out


def runs_of(roof, bmap):
    """[(y, x0, x1, plane)]: the maximal runs of equal map >= 0 and equal roof >= 1, y ascending, then x0."""
    out = []
    h, w = roof.shape
    for y in range(h):
        x = 0
        while x < w:
            if bmap[y, x] >= 0 and roof[y, x] >= 1:
                x1 = x
                while x1 + 1 < w and bmap[y, x1 + 1] == bmap[y, x] and roof[y, x1 + 1] == roof[y, x]:
                    x1 += 1
                out.append((y, x, x1, int(roof[y, x])))
                x = x1 + 1
            else:
                x += 1
    return out


def obj_text(roof, bmap, pixels, z_min, z_max, normal, center, bin, origin):
    """The text of bs_roofs_write_obj as include/bs_api.h writes it down."""
    o = [0, 0, 0] if origin is None else [int(v) for v in origin]
    runs = runs_of(np.asarray(roof), np.asarray(bmap))
    lines = [f"# roof runs: {len(runs)} over {int((np.asarray(pixels) > 0).sum())} planes"]
    for y, x0, x1, p in runs:
        for X, Y in ((x0 * bin, y * bin), ((x1 + 1) * bin, y * bin), ((x1 + 1) * bin, (y + 1) * bin), (x0 * bin, (y + 1) * bin)):
            H = int(height_of(p, X, Y, normal, center, z_min, z_max))
            lines.append(f"v {X + o[0]} {Y + o[1]} {H + o[2]}")
    for r in range(len(runs)):
        lines.append(f"f {4 * r + 1} {4 * r + 2} {4 * r + 3} {4 * r + 4}")
    return ("\n".join(lines) + "\n").encode()
