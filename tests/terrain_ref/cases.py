"""Cases of the terrain stage (include/bs_api.h, "terrain"): a building map, a cloud and the parameters each.  Every case
is a dict: name, bmap [height][width] int32, n_buildings, xyz [n][3] int32, bin, ring, q, min_ground, fallback_z.  Built once
by a fixed seed and never changed."""
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


tref = _load("terrain_ref", os.path.join(HERE, "terrain_ref.py"))
brute = tref.brute

ROOF_Z = 3000
RANK_Q = ((0, 1), (1, 2), (1, 1), (1, 3))
RANK_LOWS = ([42], [-3, 4], [10, 15, 20, 30, 30], [5, 5, 5, 7, 9, 9])  # ground_pixels 1, 2, 5, 6, with duplicates
MIN_GROUND = 8
BIG_POINTS = 600_000


def blank(w, h):
    return np.full((h, w), -1, np.int32)


def box(bmap, c, x0, x1, y0, y1):
    """pixels x0 .. x1, y0 .. y1 inclusive"""
    bmap[y0:y1 + 1, x0:x1 + 1] = c
    return bmap


def sheet(bmap, bin, seed, z_of=lambda x, y: 0 * x, per_pixel=2, skip=None, roof=True, jitter=5):
    """per_pixel points on every outside pixel (but those of `skip`) at z_of(x, y) with a jitter, and one roof point on
    every building pixel"""
    rng = np.random.default_rng(seed)
    h, w = bmap.shape
    out = (bmap < 0) if skip is None else ((bmap < 0) & ~skip)
    py, px = np.nonzero(out)
    py, px = np.repeat(py, per_pixel), np.repeat(px, per_pixel)
    x = px * bin + rng.integers(0, bin, len(px))
    y = py * bin + rng.integers(0, bin, len(py))
    z = np.asarray(z_of(x, y), np.int64) + rng.integers(-jitter, jitter + 1, len(x))
    pts = [np.stack([x, y, z], 1)]
    if roof:
        by, bx = np.nonzero(bmap >= 0)
        pts.append(np.stack([bx * bin + bin // 2, by * bin + bin // 2, np.full(len(bx), ROOF_Z)], 1))
    pts = np.concatenate(pts)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], dtype=np.int32)


def points_on(pixels_lows, bin):
    """one point per (x, y, z): in the middle of pixel (x, y)"""
    return np.array([[x * bin + bin // 2, y * bin + bin // 2, z] for x, y, z in pixels_lows], np.int32)


def case(name, bmap, xyz, ring, bin=100, q=(1, 2), min_ground=MIN_GROUND, fallback_z=0, n_buildings=None):
    nb = max(int(bmap.max()) + 1, 0) if n_buildings is None else n_buildings
    return dict(name=name, bmap=np.ascontiguousarray(bmap, np.int32), n_buildings=nb, xyz=xyz, bin=bin, ring=ring, q=q,
                min_ground=min_ground, fallback_z=fallback_z)


def ring_of(bmap, c, ring):
    """the ring pixels of building c (by the restatement of the rounds)"""
    owner, _, ringimg, _ = tref.ring_rounds(bmap, ring)
    return np.argwhere(ringimg == c)[:, ::-1].tolist()  # (x, y)


# ---- the slope scene: three boxes on a 10 % tilted sheet (also the end-to-end cloud of the device test) ---------------------
SLOPE_BOXES = ((3000, 9000, 3000, 9000), (20000, 26000, 3000, 9000), (37000, 43000, 3000, 9000))  # x0, x1, y0, y1 after the shift
SLOPE_EXTENT = (46000, 12000)
SLOPE_HEIGHT = 4000  # of every flat roof above the ground at its box's middle


def slope_ground(x):
    return np.asarray(x, np.int64) // 10


def slope_scene(seed=57):
    """three flat-roofed boxes (6 m x 6 m, 4 m high, four walls down to the ground, 17 m apart) on a sheet that rises 10 %
    along x, sampled at 200 mm and removed under the roofs.  Jittered and shuffled; already at its origin.  About 0.1 M
    points."""
    def grid(a0, a1, b0, b1, s):
        a, b = np.meshgrid(np.arange(a0, a1 + 1, s, dtype=np.int64), np.arange(b0, b1 + 1, s, dtype=np.int64), indexing="ij")
        return a.ravel(), b.ravel()
    parts = []
    gx, gy = grid(20, SLOPE_EXTENT[0] - 20, 20, SLOPE_EXTENT[1] - 20, 200)
    under = np.zeros(len(gx), bool)
    for x0, x1, y0, y1 in SLOPE_BOXES:
        under |= (gx >= x0) & (gx <= x1) & (gy >= y0) & (gy <= y1)
        top = int(slope_ground((x0 + x1) // 2)) + SLOPE_HEIGHT
        x, y = grid(x0, x1, y0, y1, 50)
        parts.append(np.stack([x, y, np.full(len(x), top)], 1))
        for yw in (y0, y1):  # (a wall runs from the ground where it stands up to the roof)
            x, t = grid(x0, x1, 0, SLOPE_HEIGHT + 300, 100)
            z = slope_ground(x) + t
            parts.append(np.stack([x, np.full(len(x), yw), z], 1)[z < top])
        for xw in (x0, x1):
            y, t = grid(y0, y1, 0, SLOPE_HEIGHT + 300, 100)
            z = slope_ground(xw) + t
            parts.append(np.stack([np.full(len(y), xw), y, z], 1)[z < top])
    parts.append(np.stack([gx[~under], gy[~under], slope_ground(gx[~under])], 1))
    pts = np.concatenate(parts)
    rng = np.random.default_rng(seed)
    pts[:, :2] += rng.integers(-10, 11, (len(pts), 2))
    pts[:, 2] += rng.integers(-5, 6, len(pts))
    pts = pts[rng.permutation(len(pts))]
    pts[:, :2] -= pts[:, :2].min(0)
    pts[:, 2] -= pts[:, 2].min()
    return np.ascontiguousarray(pts, dtype=np.int32)


def slope_map(bin):
    """every pixel that a box (with the 10 mm jitter of the scene) touches"""
    w, h = SLOPE_EXTENT[0] // bin + 1, SLOPE_EXTENT[1] // bin + 1
    bmap = blank(w, h)
    for c, (x0, x1, y0, y1) in enumerate(SLOPE_BOXES):
        box(bmap, c, (x0 - 40) // bin, (x1 + 10) // bin, (y0 - 40) // bin, (y1 + 10) // bin)
    return bmap


def build():
    cs = []
    # two buildings 3 px apart: the pixels between them reached by both in round 2 go to the lower index
    m = box(box(blank(40, 24), 0, 8, 15, 8, 15), 1, 19, 26, 8, 15)
    cs.append(case("two_close", m, sheet(m, 100, 1), ring=4))
    # a block, and an L that closes a pocket against the image's corner: only the L's own ring reaches into it
    m = box(blank(40, 32), 0, 4, 11, 6, 15)
    box(box(m, 1, 28, 29, 0, 20), 1, 28, 39, 19, 20)
    cs.append(case("corridor", m, sheet(m, 100, 2), ring=6))
    # a building in the image's corner: its ring is clipped
    m = box(blank(32, 24), 0, 0, 5, 0, 7)
    cs.append(case("border", m, sheet(m, 100, 3), ring=5))
    # one point 5 m below the sheet
    m = box(blank(32, 24), 0, 12, 19, 8, 15)
    xyz = sheet(m, 100, 4)
    cs.append(case("outlier", m, np.concatenate([xyz, points_on([(10, 10, -5000)], 100)]), ring=4))
    # the ring of building 1 holds no point
    m = box(box(blank(48, 24), 0, 6, 13, 8, 15), 1, 32, 39, 8, 15)
    empty = np.zeros(m.shape, bool)
    empty[:, 24:] = True
    cs.append(case("empty_ring", m, sheet(m, 100, 5, skip=empty), ring=4, fallback_z=-777))
    # ground_pixels exactly min_ground and one fewer
    m = box(box(blank(24, 12), 0, 5, 5, 5, 5), 1, 17, 17, 5, 5)
    pix = [(x, y, 100 + 7 * k) for k, (x, y) in enumerate(ring_of(m, 0, 2)[:MIN_GROUND])]
    pix += [(x, y, 300 + 7 * k) for k, (x, y) in enumerate(ring_of(m, 1, 2)[:MIN_GROUND - 1])]
    cs.append(case("min_ground", m, points_on(pix, 100), ring=2, fallback_z=-5))
    # the rank formula: four buildings with 1, 2, 5 and 6 ground pixels, duplicates among their lows, at four quantiles
    m = blank(40, 10)
    for c in range(4):
        box(m, c, 4 + 10 * c, 5 + 10 * c, 4, 5)
    pix = []
    for c, lows in enumerate(RANK_LOWS):
        at = ring_of(m, c, 2)
        pix += [(x, y, z) for (x, y), z in zip(at[::2], lows)]  # (every other ring pixel: some stay without a point)
        pix += [(at[0][0], at[0][1], lows[0] + 1000)]           # a second, higher point on a pixel: the minimum counts
    for qn, qd in RANK_Q:
        cs.append(case(f"ranks_{qn}_{qd}", m, points_on(pix, 100), ring=2, q=(qn, qd), min_ground=1))
    # lows on both sides of 0
    m = box(blank(32, 24), 0, 12, 19, 8, 15)
    cs.append(case("negative", m, sheet(m, 100, 8, z_of=lambda x, y: (x - 1600) * 2), ring=4))
    # more buildings than BS_TERRAIN_FIG_CAP: 1 x 1 buildings on a 3-px lattice
    m = blank(99, 96)
    ys, xs = np.mgrid[1:96:3, 1:99:3]
    m[ys.ravel(), xs.ravel()] = np.arange(ys.size, dtype=np.int32)
    cs.append(case("many", m, sheet(m, 100, 9, z_of=lambda x, y: x // 7 - y // 5, per_pixel=1, roof=False), ring=1, min_ground=4))
    # no building at all
    m = blank(16, 12)
    cs.append(case("none", m, sheet(m, 100, 10), ring=3, n_buildings=0))
    # the largest ring on an image that is full after a few rounds
    m = box(box(blank(24, 16), 0, 3, 6, 3, 6), 1, 15, 20, 8, 12)
    cs.append(case("early", m, sheet(m, 100, 11), ring=brute.MAX_RING))
    # three boxes on a 10 % tilted sheet
    cs.append(case("slope", slope_map(500), slope_scene(), ring=4, bin=500))
    return cs


CASES = build()
BY_NAME = {c["name"]: c for c in CASES}
ARGS = ("xyz", "bin", "bmap", "n_buildings", "ring", "q", "min_ground", "fallback_z")


def args(c):
    return [c[k] for k in ARGS]


def big():
    """about 600 000 points over the two_close map: more than one sweep of the pass over the points"""
    c = dict(BY_NAME["two_close"])
    h, w = c["bmap"].shape
    c["xyz"] = sheet(c["bmap"], c["bin"], 12, z_of=lambda x, y: (x * 3 + y) // 16, per_pixel=-(-BIG_POINTS // int((c["bmap"] < 0).sum())))
    c["name"] = "big"
    return c
