"""The terrain stage by its definition (include/bs_api.h, "terrain"), with Python integers: the ring as breadth-first
rounds over sets of pixels, the lows in a dict, a sorted list per building.  Nothing of the device layout is in here."""
from types import SimpleNamespace

import numpy as np

INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
MAX_RING = 255
COORD_LIMIT = 1 << 23
HEAD = ("width", "height", "n_buildings", "bin", "ring", "q_num", "q_den", "min_ground", "fallback_z")
TOTALS = ("rounds_used", "n_fallback", "n_points", "n_ring_pixels", "n_ground_pixels", "n_ring_points")
FIGURES = ("ring_pixels", "ground_pixels", "ring_points", "ground_sum", "ground_min", "ground_max", "ground", "status")
IMAGES = ("owner", "dist", "low")
FIELDS = HEAD + TOTALS + FIGURES + IMAGES


class InvalidError(ValueError):
    pass


class RangeError(ValueError):
    pass


def check(xyz, bin, bmap, n_buildings, ring, q, min_ground):
    """the errors of the definition, in the order of the library"""
    xyz, bmap = np.asarray(xyz), np.asarray(bmap)
    if len(xyz) < 1 or bin < 1 or bmap.ndim != 2 or bmap.size < 1 or bmap.size >= 2 ** 31 or n_buildings < 0:
        raise InvalidError("n, bin, the image or n_buildings")
    if not 1 <= ring <= MAX_RING or not (0 <= q[0] <= q[1] and 1 <= q[1] < 2 ** 31) or min_ground < 1:
        raise InvalidError("ring, q or min_ground")
    if len(xyz) >= 2 ** 29:
        raise RangeError("2^29 points or more")
    if int(bmap.max()) >= n_buildings:
        raise RangeError("a map value >= n_buildings")
    h, w = bmap.shape
    x, y = xyz[:, 0].astype(np.int64), xyz[:, 1].astype(np.int64)
    if (x < 0).any() or (y < 0).any() or (x // bin >= w).any() or (y // bin >= h).any():
        raise RangeError("a point outside the image")
    if (np.abs(xyz.astype(np.int64)) >= COORD_LIMIT).any():
        raise RangeError("a coordinate at or beyond 2^23")


def terrain(xyz, bin, bmap, n_buildings, ring, q=(1, 2), min_ground=8, fallback_z=0, trace=None):
    check(xyz, bin, bmap, n_buildings, ring, q, min_ground)
    h, w = np.asarray(bmap).shape
    m = [[-1 if v < 0 else int(v) for v in row] for row in np.asarray(bmap).tolist()]
    owner = [row[:] for row in m]
    dist = [[0] * w for _ in range(h)]
    rounds_used, contested = 0, 0
    for r in range(1, ring + 1):
        took = {}
        for y in range(h):
            for x in range(w):
                if owner[y][x] != -1:
                    continue
                near = {owner[v][u] for u, v in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1))
                        if 0 <= u < w and 0 <= v < h and owner[v][u] >= 0}
                if near:
                    took[y, x] = min(near)
                    contested += len(near) > 1
        for (y, x), c in took.items():  # synchronous: the round has read owner_{r-1} alone
            owner[y][x] = c
            dist[y][x] = r
        rounds_used += bool(took)
    ring_pixel = [[m[y][x] == -1 and owner[y][x] >= 0 for x in range(w)] for y in range(h)]
    low = [[INT32_MAX] * w for _ in range(h)]
    ring_points = [0] * n_buildings
    for x, y, z in np.asarray(xyz).tolist():
        px, py = x // bin, y // bin
        if ring_pixel[py][px]:
            low[py][px] = min(low[py][px], z)
            ring_points[owner[py][px]] += 1
    G = [[] for _ in range(n_buildings)]
    ring_pixels = [0] * n_buildings
    for y in range(h):
        for x in range(w):
            if ring_pixel[y][x]:
                ring_pixels[owner[y][x]] += 1
                if low[y][x] != INT32_MAX:
                    G[owner[y][x]].append(low[y][x])
    ground, status = [], []
    for g in G:
        g.sort()
        if len(g) >= min_ground:
            ground.append(g[(len(g) - 1) * q[0] // q[1]])
            status.append(0)
        else:
            ground.append(fallback_z)
            status.append(1)
    if trace is not None:
        trace["contested"] = contested
    i64, i32 = np.int64, np.int32
    return SimpleNamespace(
        width=w, height=h, n_buildings=n_buildings, bin=bin, ring=ring, q_num=q[0], q_den=q[1], min_ground=min_ground,
        fallback_z=fallback_z, rounds_used=rounds_used, n_fallback=sum(status), n_points=len(xyz), n_ring_pixels=sum(ring_pixels),
        n_ground_pixels=sum(len(g) for g in G), n_ring_points=sum(ring_points), ring_pixels=np.array(ring_pixels, i64),
        ground_pixels=np.array([len(g) for g in G], i64), ring_points=np.array(ring_points, i64),
        ground_sum=np.array([sum(g) for g in G], i64), ground_min=np.array([g[0] if g else INT32_MAX for g in G], i32),
        ground_max=np.array([g[-1] if g else INT32_MIN for g in G], i32), ground=np.array(ground, i32), status=np.array(status, i32),
        owner=np.array(owner, i32).reshape(h, w), dist=np.array(dist, np.uint8).reshape(h, w), low=np.array(low, i32).reshape(h, w))


def same(a, b, fields=FIELDS):
    """None, or the name of the first field in which the two results differ"""
    for k in fields:
        u, v = getattr(a, k), getattr(b, k)
        if isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
            u, v = np.asarray(u), np.asarray(v)
            if u.shape != v.shape or u.dtype != v.dtype or not np.array_equal(u, v):
                return k
        elif u != v:
            return k
    return None


def l1_to_owner(bmap, owner):
    """per pixel the L1 distance to the nearest pixel of the building in `owner` (-1 where owner < 0), by brute force"""
    bmap, owner = np.asarray(bmap), np.asarray(owner)
    h, w = bmap.shape
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.full((h, w), -1, np.int64)
    for c in np.unique(owner[owner >= 0]).tolist():
        by, bx = np.nonzero(bmap == c)
        sel = owner == c
        d = np.abs(yy[sel][:, None] - by[None, :]) + np.abs(xx[sel][:, None] - bx[None, :])
        out[sel] = d.min(1)
    return out
