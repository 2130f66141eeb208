"""Cases of the roof evidence (include/bs_api.h, "roof evidence").  Every case is a dict: name, xyz [n][3] int32, plane_idx [n]
int32, n_planes, plane_ok (uint8 [n_planes] or None), extent [3] int32, bin, ground_th, params (brute.params), model ((dtm,
cell, min_height) or None).  Built by fixed seeds and never changed.  CASES are small enough for the brute force; LARGE are
for the restatement alone.  tree_scene() is the premise: the three boxes of tests/ground_ref with tree crowns."""
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


eref = _load("evidence_ref", os.path.join(HERE, "evidence_ref.py"))
brute, gref = eref.brute, eref.gref
gcases = _load("ground_cases", os.path.join(os.path.dirname(HERE), "ground_ref", "cases.py"))
EMPTY = brute.EMPTY
TILE = 32    # BS_EVIDENCE_TILE
GRID = 256   # BS_EVIDENCE_GRID
BIN = 100


def extent_of(w, h, bin=BIN, zmax=0):
    """an extent whose lattice is w x h"""
    return np.array([(w - 2) * bin, (h - 2) * bin, zmax], np.int32)


def noise(name, w, h, n, seed, r=3, min_points=1, share=(1, 2), n_planes=5, ok=(1, 0, 1, 1, 0), fill=0.6, bin=BIN,
          ground_th=1000.0, zmax=3000, model=None, hot=0, scan_tail=0):
    """n points over a random `fill` of the pixels of a w x h lattice, a third of them below ground, labels -1 .. n_planes + 1;
    the first `hot` of them in one pixel; the last `scan_tail` of them in scan order (sorted by pixel: runs of equal pixels,
    with points below ground and of rejected planes inside the runs)"""
    rng = np.random.default_rng(seed)
    live = np.nonzero(rng.random(w * h) < fill)[0]
    if len(live) == 0:
        live = np.array([0])
    pix = live[rng.integers(0, len(live), n)]
    pix[:hot] = live[len(live) // 2]
    if scan_tail:
        pix[n - scan_tail:] = np.sort(pix[n - scan_tail:])
    x = (pix % w) * bin + rng.integers(0, bin, n)
    y = (pix // w) * bin + rng.integers(0, bin, n)
    z = rng.integers(0, zmax, n)
    lab = rng.integers(-1, n_planes + 2, n)
    return dict(name=name, xyz=np.ascontiguousarray(np.stack([x, y, z], 1), np.int32), plane_idx=lab.astype(np.int32),
                n_planes=n_planes, plane_ok=None if ok is None else np.array(ok, np.uint8), extent=extent_of(w, h, bin, zmax),
                bin=bin, ground_th=float(ground_th), params=brute.params(r, min_points, share), model=model)


def points(name, w, h, pts, r=0, min_points=1, share=(1, 2), n_planes=1, ok=None, ground_th=0.0, model=None):
    """hand-placed points (pixel x, pixel y, z, label), each at the middle of its pixel"""
    a = np.array([(px * BIN + 50, py * BIN + 50, z) for px, py, z, _ in pts], np.int32).reshape(-1, 3)
    return dict(name=name, xyz=a, plane_idx=np.array([p[3] for p in pts], np.int32), n_planes=n_planes,
                plane_ok=None if ok is None else np.array(ok, np.uint8), extent=extent_of(w, h), bin=BIN,
                ground_th=float(ground_th), params=brute.params(r, min_points, share), model=model)


# where the hand-made cases put what they are there for (pixels x, y)
BOUNDARY_KEPT, BOUNDARY_DROPPED = (1, 1), (4, 1)   # 2 of 4 planar: exactly 1/2; 2 of 5: under it
THIN_AT = (2, 2)                                    # three points in one pixel


def tilted_model(w, h, cell=200):
    """a dtm over the lattice of `cell` that rises along x, with an EMPTY entry, and that ends before the last columns"""
    gw, gh = max(1, (w * BIN) // cell - 2), (h * BIN) // cell + 1
    dtm = (np.arange(gw, dtype=np.int64)[None, :] * 150 + np.zeros((gh, 1), np.int64)).astype(np.int32)
    dtm[gh // 2, gw // 2] = EMPTY
    return dtm, cell, 800


def build():
    cs = [points("one_point", 2, 2, [(0, 0, 5, 1)])]
    cs.append(noise("r0", 20, 14, 900, 1, r=0))
    cs.append(noise("r1", 20, 14, 900, 2, r=1))
    cs.append(noise("scan_order", 20, 14, 900, 11, r=1, scan_tail=900))  # about five points a pixel: a dozen runs in a wave
    cs.append(noise("r15_narrow", 9, 40, 1200, 3, r=15, share=(2, 5)))
    cs.append(noise("straddle_small", 36, 35, 2500, 4, r=3))   # 2 x 2 tiles of 32: the windows around (32, 32) straddle four
    cs.append(noise("no_planes", 12, 10, 400, 5, r=2, n_planes=0, ok=None))
    cs.append(noise("every_plane", 12, 10, 400, 6, r=2, ok=None))
    cs.append(noise("num_zero", 12, 10, 400, 7, r=1, share=(0, 3)))
    # every point of the window must be planar: (1, 1) holds two of plane 1, (4, 1) one of them and one unlabelled point
    cs.append(points("num_is_den", 7, 4, [(1, 1, 5, 1), (1, 1, 5, 1), (4, 1, 5, 1), (4, 1, 5, 0)], share=(3, 3)))
    cs.append(noise("all_below", 12, 10, 400, 9, r=2, ground_th=1e9))
    # labels 0, -1 and n_planes + 1 are unlabelled; plane 2 fails the table
    cs.append(points("labels", 8, 4, [(1, 1, 5, 0), (2, 1, 5, -1), (3, 1, 5, 3), (4, 1, 5, 1), (5, 1, 5, 2)], n_planes=2, ok=(1, 0),
                     share=(1, 1)))
    pts = [(BOUNDARY_KEPT[0], BOUNDARY_KEPT[1], 5, lab) for lab in (1, 1, 0, 0)]
    pts += [(BOUNDARY_DROPPED[0], BOUNDARY_DROPPED[1], 5, lab) for lab in (1, 1, 0, 0, 0)]
    cs.append(points("share_boundary", 7, 4, pts))
    three = [(THIN_AT[0], THIN_AT[1], 5, 1)] * 3
    cs.append(points("min_points_at", 6, 6, three, r=1, min_points=3))
    cs.append(points("min_points_over", 6, 6, three, r=1, min_points=4))
    cs.append(noise("model", 22, 12, 1500, 10, r=2, ground_th=1500.0, model=tilted_model(22, 12)))
    return cs


CASES = build()
BY_NAME = {c["name"]: c for c in CASES}


def large():
    """the shapes at which the kernels can go wrong, too large for the brute force"""
    cs = [noise("tile_minus", TILE - 1, TILE - 1, 4000, 20, r=2), noise("tile_plus", TILE + 1, TILE + 1, 4000, 21, r=2),
          noise("tile_exact", TILE, TILE, 4000, 22, r=15), noise("wide", 700, 3, 6000, 23, r=3), noise("tall", 3, 700, 6000, 24, r=3),
          noise("four_tiles", 70, 70, 20000, 25, r=7, fill=0.9), noise("sweep_pixels", 600, 600, 200000, 26, r=3, fill=0.3),
          sweep_points(),
          noise("model_large", 90, 50, 30000, 28, r=3, ground_th=1500.0, model=tilted_model(90, 50))]
    return cs


SWEEP = 256 * 2048        # the points of one sweep of the counts pass: 256 x BS_GROUND_GRID
SWEEP_POINTS = 600_037    # more than one sweep; the second sweep ends inside a wave (75 749 = 1 183 x 64 + 37)
SWEEP_SCAN_TAIL = 120_000  # in scan order, the whole second sweep included


def sweep_points():
    """more points than one sweep of the counts pass on a 40 x 40 lattice: 9 000 points on one pixel at the front, and the last
    120 000 in scan order, so every thread's second point lies in a run of equal pixels and the last wave is partly idle"""
    return noise("sweep_points", 40, 40, SWEEP_POINTS, 27, r=3, fill=0.8, hot=9000, scan_tail=SWEEP_SCAN_TAIL)


def args(c):
    return (c["xyz"], c["plane_idx"], c["n_planes"], c["plane_ok"], c["extent"], c["bin"], c["ground_th"], c["params"], c["model"])


# ---- the premise: boxes and trees -------------------------------------------------------------------------------------------
# crowns: (x, y of the middle, horizontal radius), all between 2 and 8 m above the ground; the first stands free between box 0
# and box 1, the third reaches 0.7 m over the east wall of box 1, the second touches the third
CROWNS = ((14500, 6000, 2500), (31500, 6200, 2000), (27800, 6000, 2500))
CROWN_Z = (2000, 8000)
CROWN_POINTS = (10000, 9000, 10000)
_TREE = {}


SLOPE_WALL_DZ, SLOPE_SEED = 300, 63


def slope_scene(rise, wall_dz=SLOPE_WALL_DZ, seed=SLOPE_SEED):
    """tests/ground_ref/cases.dense_slope_scene with its walls sampled every `wall_dz` mm in height (there: 100) and its own
    shuffle.  At 100 mm a wall pixel holds 26 unlabelled points above the ground model's 2 m against 4 roof points a pixel,
    and within r = 3 of the wall line the share of planar points falls under 1/2; at 300 mm it holds 9.  The seed is chosen:
    the grower leaves the neighbours of failed seeds under the next plane's label, a dozen such points 4 m away lift a roof's
    rms residual over 100 mm, and which plane they fall to depends on the order of the cloud ("Roof evidence",
    has the seeds tried)."""
    boxes, extent, height = gcases.SLOPE_BOXES, gcases.SLOPE_EXTENT, gcases.SLOPE_HEIGHT

    def ground_z(x):
        return np.asarray(x, np.int64) * rise // 1000

    def grid(a0, a1, b0, b1, sa, sb=None):
        a, b = np.meshgrid(np.arange(a0, a1 + 1, sa, dtype=np.int64), np.arange(b0, b1 + 1, sb or sa, dtype=np.int64), indexing="ij")
        return a.ravel(), b.ravel()
    parts = []
    gx, gy = grid(20, extent[0] - 20, 20, extent[1] - 20, 100)
    under = np.zeros(len(gx), bool)
    for x0, x1, y0, y1 in boxes:
        under |= (gx >= x0) & (gx <= x1) & (gy >= y0) & (gy <= y1)
        top = int(ground_z((x0 + x1) // 2)) + height
        x, y = grid(x0, x1, y0, y1, 50)
        parts.append(np.stack([x, y, np.full(len(x), top)], 1))
        for yw in (y0, y1):
            x, t = grid(x0, x1, 0, height + 600, 100, wall_dz)
            z = ground_z(x) + t
            parts.append(np.stack([x, np.full(len(x), yw), z], 1)[z < top])
        for xw in (x0, x1):
            y, t = grid(y0, y1, 0, height + 600, 100, wall_dz)
            z = ground_z(xw) + t
            parts.append(np.stack([np.full(len(y), xw), y, z], 1)[z < top])
    parts.append(np.stack([gx[~under], gy[~under], ground_z(gx[~under])], 1))
    pts = np.concatenate(parts)
    rng = np.random.default_rng(seed)
    pts[:, :2] += rng.integers(-10, 11, (len(pts), 2))
    pts[:, 2] += rng.integers(-5, 6, len(pts))
    pts = pts[rng.permutation(len(pts))]
    pts[:, :2] -= pts[:, :2].min(0)
    pts[:, 2] -= pts[:, 2].min()
    return np.ascontiguousarray(pts, dtype=np.int32)


def tree_scene(rise=0):
    """(xyz [n][3] int32, is_tree bool [n]): the three boxes -- tests/ground_ref/cases.scene(0) on the level, slope_scene(rise)
    on a slope -- and random points in the crowns' ellipsoids, shuffled; the crowns stay inside the scene's extent in x and
    y, so its lattice and its truth map are the scene's"""
    if rise not in _TREE:
        base = gcases.scene(0) if rise == 0 else slope_scene(rise)
        rng = np.random.default_rng(97)
        parts, zc, zr = [base], sum(CROWN_Z) // 2, (CROWN_Z[1] - CROWN_Z[0]) // 2
        for (cx, cy, rad), m in zip(CROWNS, CROWN_POINTS):
            u = rng.normal(size=(m, 3))
            u *= (rng.random(m) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
            ground = cx * rise // 1000
            parts.append(np.stack([cx + u[:, 0] * rad, cy + u[:, 1] * rad, ground + zc + u[:, 2] * zr], 1).astype(np.int64))
        pts = np.concatenate(parts)
        tree = np.arange(len(pts)) >= len(base)
        order = rng.permutation(len(pts))
        xyz = np.ascontiguousarray(pts[order], np.int32)
        assert (xyz.min(0) >= 0).all() and (xyz[:, :2].max(0) == base[:, :2].max(0)).all()
        xyz.setflags(write=False)
        _TREE[rise] = (xyz, tree[order])
    return _TREE[rise]


def truth_map():
    return gcases.slope_map(BIN)
