"""CPU restatement of the building map, the point assignment, the plane votes and the LoD1 OBJ (include/bs_api.h,
"buildings") that the building tests compare the device against.  numpy + scipy, in another formulation than the
device's: scipy.ndimage.label twice (no union-find), bincount / reduceat for the figures, a dense count matrix for
the votes."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
FOUR = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
EIGHT = np.ones((3, 3), int)
# the per-building arrays of building_map and of assign, under the names the device's Buildings gives them
PIXEL_FIGURES = ("start_xy", "bbox", "pixels", "fg_pixels")
POINT_FIGURES = ("n_points", "n_above", "z_min", "z_max", "z_sum")


def _per_group(keys, n_groups):
    """(order, first, present): a stable order that groups equal keys, the first position of every present group in
    it, and the present groups -- for ufunc.reduceat."""
    order = np.argsort(keys, kind="stable")
    present, first = np.unique(keys[order], return_index=True)
    return order, first, present


def building_map(mask):
    """map int32 [h][w] and the pixel figures of a closed mask (non-zero = foreground)."""
    import scipy.ndimage as nd
    m = np.asarray(mask) != 0
    h, w = m.shape
    p = np.pad(m, 1)
    bg, _ = nd.label(~p, structure=FOUR)
    filled = bg != bg[0, 0]  # not the frame's background region: foreground and everything it encloses
    lab, n = nd.label(filled, structure=EIGHT)
    flat = lab.ravel()
    idx = np.flatnonzero(flat)
    labs, first = np.unique(flat[idx], return_index=True)
    starts = idx[first]  # first pixel of every label in raster order
    order = np.argsort(-starts, kind="stable")  # building c = the c-th largest start pixel
    rank = np.full(n + 1, -1, np.int32)
    rank[labs[order]] = np.arange(n, dtype=np.int32)
    bmap = np.ascontiguousarray(rank[lab][1:-1, 1:-1])
    wp = w + 2
    s = starts[order]
    out = SimpleNamespace(n_buildings=n, width=w, height=h, map=bmap,
                          start_xy=np.stack([s % wp - 1, s // wp - 1], 1).astype(np.int32).reshape(n, 2))
    ys, xs = np.nonzero(bmap >= 0)
    b = bmap[ys, xs]
    out.pixels = np.bincount(b, minlength=n).astype(np.int64)
    out.fg_pixels = np.bincount(bmap[m & (bmap >= 0)], minlength=n).astype(np.int64)
    out.bbox = np.zeros((n, 4), np.int32)
    if n:
        o, f, present = _per_group(b, n)
        assert len(present) == n
        out.bbox[:, 0] = np.minimum.reduceat(xs[o], f)
        out.bbox[:, 1] = np.minimum.reduceat(ys[o], f)
        out.bbox[:, 2] = np.maximum.reduceat(xs[o], f)
        out.bbox[:, 3] = np.maximum.reduceat(ys[o], f)
    return out


def enclosed_pixels(mask, bmap):
    """Pixels that belong to a building without being foreground (holes and what lies in them that is background)."""
    return (np.asarray(bmap) >= 0) & (np.asarray(mask) == 0)


def assign(xyz, bmap, n_buildings, bin, ground_th):
    """building_idx and the point figures; raises IndexError if a pixel lies outside the image."""
    xyz = np.asarray(xyz, dtype=np.int64)
    h, w = bmap.shape
    if (xyz[:, :2] < 0).any():
        raise IndexError("negative coordinate")
    px, py = xyz[:, 0] // bin, xyz[:, 1] // bin
    if (px >= w).any() or (py >= h).any():
        raise IndexError("pixel outside the image")
    bidx = bmap[py, px].astype(np.int32)
    n = n_buildings
    above = ~(xyz[:, 2].astype(np.float64) < ground_th)
    out = SimpleNamespace(building_idx=bidx, above=above)
    out.n_points = np.bincount(bidx[bidx >= 0], minlength=n).astype(np.int64)
    sel = above & (bidx >= 0)
    out.n_above = np.bincount(bidx[sel], minlength=n).astype(np.int64)
    out.z_min = np.full(n, I32_MAX, np.int32)
    out.z_max = np.full(n, I32_MIN, np.int32)
    out.z_sum = np.zeros(n, np.int64)
    if sel.any():
        z = xyz[sel, 2]
        o, f, present = _per_group(bidx[sel], n)
        out.z_min[present] = np.minimum.reduceat(z[o], f)
        out.z_max[present] = np.maximum.reduceat(z[o], f)
        out.z_sum[present] = np.add.reduceat(z[o], f)
    return out


def votes(plane_idx, building_idx, n_planes, n_buildings):
    """(plane_building, votes_in, votes_total, votes_outside), entry p - 1 = plane p."""
    p = np.asarray(plane_idx, dtype=np.int64)
    b = np.asarray(building_idx, dtype=np.int64)
    sel = (p >= 1) & (p <= n_planes)
    cols = n_buildings + 1
    counts = np.bincount((p[sel] - 1) * cols + b[sel] + 1, minlength=n_planes * cols).reshape(n_planes, cols)
    total = counts.sum(1).astype(np.int64)
    outside = counts[:, 0].astype(np.int64)
    if n_buildings:
        inside = counts[:, 1:]
        win = inside.argmax(1)  # the first maximum: ties go to the lower index
        vin = inside[np.arange(n_planes), win].astype(np.int64)
        pb = np.where(vin > 0, win, -1).astype(np.int32)
    else:
        vin, pb = np.zeros(n_planes, np.int64), np.full(n_planes, -1, np.int32)
    return pb, vin, total, outside


def _tdiv(a, b):
    """C's integer division: the quotient truncated towards zero."""
    q = abs(int(a)) // abs(int(b))
    return q if (a < 0) == (b < 0) else -q


def obj_text(contours, area, perimeter, n_above, z_sum, bin, origin, ground_th, min_area=500.0, min_perimeter=100.0):
    """The text of bs_buildings_write_obj as include/bs_api.h writes it down."""
    o = [0, 0, 0] if origin is None else [int(v) for v in origin]
    kept = [i for i in range(len(contours))
            if area[i] > min_area and perimeter[i] > min_perimeter and n_above[i] > 0]
    lines = [f"# buildings: {len(kept)} of {len(contours)}"]
    z0 = int(ground_th) + o[2]  # int() truncates towards zero like the C cast
    for i in kept:
        z1 = _tdiv(z_sum[i], n_above[i]) + o[2]
        for x, y in contours[i]:
            X, Y = int(x) * bin + o[0], int(y) * bin + o[1]
            lines += [f"v {X} {Y} {z0}", f"v {X} {Y} {z1}"]
    base = 1
    for i in kept:
        n = len(contours[i])
        for k in range(n):
            nx = (k + 1) % n
            lines.append(f"f {base + 2 * k} {base + 2 * nx} {base + 2 * nx + 1} {base + 2 * k + 1}")
        base += 2 * n
    base = 1
    for i in kept:
        n = len(contours[i])
        if n >= 3:
            lines.append("f " + " ".join(str(base + 2 * k + 1) for k in range(n)))
        base += 2 * n
    return ("\n".join(lines) + "\n").encode()
