"""The terrain stage as the device lays it out (buildingsegment_amd/csrc/bs_terrain.hip), restated in numpy: frontier
worklists with a push (a minimum into `next`) and a commit per round, the ring image that the pass over the points gathers
from, a minimum into `low` for the points on ring pixels alone, the 64-bit keys (building << 32) | (low ^ 0x80000000) of the
ring pixels that hold a point, one sort of them, the exclusive sum of ground_pixels and one pick per building."""
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


brute = _load("terrain_brute", os.path.join(HERE, "brute.py"))

INT32_MAX, INT32_MIN = brute.INT32_MAX, brute.INT32_MIN
MAX_RING = 255    # BS_TERRAIN_MAX_RING of include/bs_api.h
FIG_CAP = 1024    # BS_TERRAIN_FIG_CAP
GRID = 2048       # BS_TERRAIN_GRID
DEVICE_FIELDS = brute.FIELDS + ("fig_cap", "grid")


def ring_rounds(bmap, ring, trace=None):
    """(owner, dist, ring image, rounds_used) by frontier lists"""
    h, w = bmap.shape
    m = np.where(bmap < 0, -1, bmap).astype(np.int32).ravel()
    owner, ringimg = m.copy(), np.full(h * w, -1, np.int32)
    nxt = np.full(h * w, INT32_MAX, np.int32)
    dist = np.zeros(h * w, np.uint8)
    out2 = m.reshape(h, w) < 0
    front = np.zeros((h, w), bool)  # the building pixels with an outside 4-neighbour
    front[:, 1:] |= out2[:, :-1]
    front[:, :-1] |= out2[:, 1:]
    front[1:, :] |= out2[:-1, :]
    front[:-1, :] |= out2[1:, :]
    cur = np.flatnonzero(front.ravel() & (m >= 0))
    rounds_used, lists = 0, [len(cur)]
    for r in range(1, ring + 1):
        if len(cur) == 0:
            break  # (the kernels leave at once on an empty list)
        y, x = cur // w, cur % w
        o = owner[cur]
        reached = []
        for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
            nx, ny = x + dx, y + dy
            ok = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
            q = (ny * w + nx)[ok]
            free = owner[q] == -1
            np.minimum.at(nxt, q[free], o[ok][free])  # the push: owner is only read
            reached.append(q[free])
        cur = np.unique(np.concatenate(reached))  # the first pusher lists the pixel: once
        owner[cur] = nxt[cur]  # the commit
        ringimg[cur] = nxt[cur]
        dist[cur] = r
        rounds_used += len(cur) > 0
        lists.append(len(cur))
    if trace is not None:
        trace["lists"] = lists
    return owner.reshape(h, w), dist.reshape(h, w), ringimg.reshape(h, w), rounds_used


def terrain(xyz, bin, bmap, n_buildings, ring, q=(1, 2), min_ground=8, fallback_z=0, trace=None):
    brute.check(xyz, bin, bmap, n_buildings, ring, q, min_ground)
    xyz, bmap = np.asarray(xyz, np.int32), np.asarray(bmap, np.int32)
    h, w = bmap.shape
    nb, n = n_buildings, len(xyz)
    if nb > 0:
        owner, dist, ringimg, rounds_used = ring_rounds(bmap, ring, trace)
    else:
        owner, dist, ringimg, rounds_used = np.full((h, w), -1, np.int32), np.zeros((h, w), np.uint8), np.full((h, w), -1, np.int32), 0
    # the points: one gather from the ring image, a minimum for the points on ring pixels alone
    p = (xyz[:, 1] // bin).astype(np.int64) * w + xyz[:, 0] // bin
    c = ringimg.ravel()[p]
    on = c >= 0
    low = np.full(h * w, INT32_MAX, np.int32)
    np.minimum.at(low, p[on], xyz[on, 2])
    ring_points = np.bincount(c[on], minlength=nb).astype(np.int64)[:nb] if nb else np.zeros(0, np.int64)
    # the pixels: keys and figures
    rp = np.flatnonzero(ringimg.ravel() >= 0)
    rc, rl = ringimg.ravel()[rp].astype(np.int64), low[rp]
    has = rl != INT32_MAX
    keys = (rc[has].astype(np.uint64) << np.uint64(32)) | (rl[has].astype(np.int64) + 2 ** 31).astype(np.uint64)  # (low ^ 0x80000000)
    ring_pixels = np.bincount(rc, minlength=nb).astype(np.int64)[:nb] if nb else np.zeros(0, np.int64)
    ground_pixels = np.bincount(rc[has], minlength=nb).astype(np.int64)[:nb] if nb else np.zeros(0, np.int64)
    ground_sum, ground_min, ground_max = np.zeros(nb, np.int64), np.full(nb, INT32_MAX, np.int32), np.full(nb, INT32_MIN, np.int32)
    np.add.at(ground_sum, rc[has], rl[has].astype(np.int64))
    np.minimum.at(ground_min, rc[has], rl[has])
    np.maximum.at(ground_max, rc[has], rl[has])
    # the pick
    srt = np.sort(keys)
    off = np.concatenate([[0], np.cumsum(ground_pixels)])[:nb].astype(np.int64)
    ok = ground_pixels >= min_ground
    at = off + (ground_pixels - 1) * q[0] // q[1]
    ground, status = np.full(nb, fallback_z, np.int32), np.ones(nb, np.int32)
    if ok.any():
        k = srt[at[ok]]
        assert ((k >> np.uint64(32)).astype(np.int64) == np.flatnonzero(ok)).all()
        ground[ok] = ((k & np.uint64(0xFFFFFFFF)).astype(np.int64) - 2 ** 31).astype(np.int32)
        status[ok] = 0
    if trace is not None:
        trace["n_keys"] = int(len(keys))
        trace["second_point_threads"] = max(n - GRID * 256, 0)
        trace["lds_buildings"] = int((ring_pixels[:FIG_CAP] > 0).sum())
        trace["atomic_buildings"] = int((ring_pixels[FIG_CAP:] > 0).sum())
    return SimpleNamespace(
        width=w, height=h, n_buildings=nb, bin=bin, ring=ring, q_num=q[0], q_den=q[1], min_ground=min_ground, fallback_z=fallback_z,
        fig_cap=FIG_CAP, grid=GRID, rounds_used=rounds_used, n_fallback=int(status.sum()), n_points=n,
        n_ring_pixels=int(ring_pixels.sum()), n_ground_pixels=int(ground_pixels.sum()), n_ring_points=int(ring_points.sum()),
        ring_pixels=ring_pixels, ground_pixels=ground_pixels, ring_points=ring_points, ground_sum=ground_sum, ground_min=ground_min,
        ground_max=ground_max, ground=ground, status=status, owner=owner, dist=dist, low=low.reshape(h, w))


def same(a, b, fields=DEVICE_FIELDS):
    return brute.same(a, b, fields)
