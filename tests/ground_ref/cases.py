"""Cases of the ground stage (include/bs_api.h, "ground"): a cloud, an extent and the parameters each.  Every case is a dict:
name, xyz [n][3] int32, extent [3] int32, params (tests/ground_ref/ground_ref.params).  Built once by fixed seeds and never
changed.  A lattice is bs_grid_dims(extent, cell), so it has at least two rows and two columns: `row` and `column` hold
their points in one line of 300 pixels and leave the second line EMPTY."""
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


gref = _load("ground_ref", os.path.join(HERE, "ground_ref.py"))
brute = gref.brute
tcases = _load("terrain_cases", os.path.join(os.path.dirname(HERE), "terrain_ref", "cases.py"))
EMPTY = gref.EMPTY
SLOPE_BOXES, SLOPE_EXTENT, SLOPE_HEIGHT, slope_map = tcases.SLOPE_BOXES, tcases.SLOPE_EXTENT, tcases.SLOPE_HEIGHT, tcases.slope_map
BIG_POINTS = 600_000
Z_LIMIT = (1 << 23) - 1


def extent_of(w, h, cell, zmax=0):
    """an extent whose lattice is w x h"""
    return np.array([(w - 2) * cell, (h - 2) * cell, max(int(zmax), 0)], np.int32)


def cloud(low, cell, seed, extra=1):
    """one point at z = low in every pixel whose low is not EMPTY (anywhere inside the pixel), and `extra` higher ones"""
    rng = np.random.default_rng(seed)
    py, px = np.nonzero(low != EMPTY)
    z0 = low[py, px].astype(np.int64)
    parts = []
    for j in range(1 + extra):
        x = px * cell + rng.integers(0, cell, len(px))
        y = py * cell + rng.integers(0, cell, len(py))
        z = z0 if j == 0 else np.minimum(z0 + rng.integers(0, 400, len(px)), Z_LIMIT)
        parts.append(np.stack([x, y, z], 1))
    pts = np.concatenate(parts)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], dtype=np.int32)


def relief(w, h, seed, boxes=3, amp=40, box_height=(2500, 6000)):
    """a tilted, rough sheet with a few raised boxes: int64 [h][w]"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    z = xs * int(rng.integers(-30, 31)) + ys * int(rng.integers(-30, 31)) + rng.integers(-amp, amp + 1, (h, w))
    for _ in range(boxes):
        bw, bh = int(rng.integers(1, max(2, w // 3))), int(rng.integers(1, max(2, h // 3)))
        x0, y0 = int(rng.integers(0, max(1, w - bw))), int(rng.integers(0, max(1, h - bh)))
        z[y0:y0 + bh, x0:x0 + bw] += int(rng.integers(*box_height))
    return z.astype(np.int64)


def case(name, low, cell, seed, extra=1, xyz=None, **kw):
    h, w = low.shape
    p = gref.params(cell=cell, **kw)
    xyz = cloud(low, cell, seed, extra) if xyz is None else xyz
    return dict(name=name, xyz=xyz, extent=extent_of(w, h, cell, xyz[:, 2].max()), params=p)


def threshold_of(cell, r, prev=0, slope=(3, 10), dh0=200, dh_max=2500):
    return min(dh_max, dh0 + slope[0] * (r - prev) * cell // slope[1])


# ---- the dense tilted scene: the three boxes of the terrain's slope scene, the ground as an airborne scan samples it -------
def dense_slope_scene(rise, seed=61):
    """the boxes and the extent of tests/terrain_ref/cases.slope_scene on a sheet that rises `rise` mm per metre along x,
    sampled at 100 mm and removed under the roofs; flat roofs SLOPE_HEIGHT above the ground at their box's middle, roofs at
    50 mm, four walls from the ground where they stand (at most SLOPE_HEIGHT + 600 high) at 100 mm.  Jittered, shuffled, at
    its origin.  About 0.12 M points."""
    def ground_z(x):
        return np.asarray(x, np.int64) * rise // 1000

    def grid(a0, a1, b0, b1, s):
        a, b = np.meshgrid(np.arange(a0, a1 + 1, s, dtype=np.int64), np.arange(b0, b1 + 1, s, dtype=np.int64), indexing="ij")
        return a.ravel(), b.ravel()
    parts = []
    gx, gy = grid(20, SLOPE_EXTENT[0] - 20, 20, SLOPE_EXTENT[1] - 20, 100)
    under = np.zeros(len(gx), bool)
    for x0, x1, y0, y1 in SLOPE_BOXES:
        under |= (gx >= x0) & (gx <= x1) & (gy >= y0) & (gy <= y1)
        top = int(ground_z((x0 + x1) // 2)) + SLOPE_HEIGHT
        x, y = grid(x0, x1, y0, y1, 50)
        parts.append(np.stack([x, y, np.full(len(x), top)], 1))
        for yw in (y0, y1):
            x, t = grid(x0, x1, 0, SLOPE_HEIGHT + 600, 100)
            z = ground_z(x) + t
            parts.append(np.stack([x, np.full(len(x), yw), z], 1)[z < top])
        for xw in (x0, x1):
            y, t = grid(y0, y1, 0, SLOPE_HEIGHT + 600, 100)
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


_SCENES = {}


def scene(rise):
    if rise not in _SCENES:
        _SCENES[rise] = dense_slope_scene(rise)
        _SCENES[rise].setflags(write=False)
    return _SCENES[rise]


def scene_case(rise, cell=500):
    xyz = scene(rise)
    return dict(name=f"slope_{rise}", xyz=xyz, extent=xyz.max(0).astype(np.int32), params=gref.params(cell=cell))


# where the cases put what they are there for (pixels x, y): the tests read these
EDGE_EQUAL, EDGE_OVER = (6, 6), (16, 6)   # the middles of two 3 x 3 plateaus of exactly t_1 and t_1 + 1
SPIKE, PLATEAU = (12, 10), (10, 8, 14, 12)  # a spike on a 5 x 5 plateau (x0, y0, x1, y1 inclusive)
CAP_PLATEAU = (14, 10, 25, 21)              # the 12 x 12 plateau of `cap` (x0, y0, x1, y1 inclusive)
HOLE = (16, 14, 55, 49)                    # the EMPTY region of `hole` (x0, y0, x1, y1 inclusive)


def build():
    cs = []
    cs.append(case("tiny", relief(24, 16, 1), 100, 1, radius=[1]))
    cs.append(case("wide_window", relief(24, 16, 2), 100, 2, radius=[255]))
    low = relief(300, 2, 3, boxes=4)
    low[1, :] = EMPTY
    cs.append(case("row", low, 100, 3, radius=[1, 2, 5, 40]))
    low = relief(2, 300, 4, boxes=4)
    low[:, 1] = EMPTY
    cs.append(case("column", low, 100, 4, radius=[1, 2, 5, 40]))
    cs.append(case("odd", relief(131, 67, 5, boxes=6), 100, 5, radius=[1, 3, 7, 20]))
    # rows longer than one row segment of the x passes (BS_GROUND_ROW_LDS - 2 r outputs: 2046, 1988 and 1538 of them)
    cs.append(case("long_rows", relief(2100, 3, 13, boxes=9, amp=300), 10, 13, radius=[1, 30, 255]))
    # an EMPTY region larger than the largest window: a step fills 2 r pixels inwards, 14 in all, of 20 and 18 to the middle
    low = relief(72, 64, 6)
    low[HOLE[1]:HOLE[3] + 1, HOLE[0]:HOLE[2] + 1] = EMPTY
    cs.append(case("hole", low, 100, 6, radius=[1, 2, 4]))
    # a step of exactly t_1 and one of t_1 + 1 on a level sheet: 3 x 3 plateaus, which the 5 x 5 window removes
    t1 = threshold_of(100, 2)
    low = np.zeros((14, 24), np.int64)
    for (x, y), top in ((EDGE_EQUAL, t1), (EDGE_OVER, t1 + 1)):
        low[y - 1:y + 2, x - 1:x + 2] = top
    cs.append(case("edge_equal", low, 100, 7, extra=0, radius=[2]))
    # a spike on a plateau: the 3 x 3 window removes the spike (step 1), the 7 x 7 window the plateau under it (step 2), and
    # the spike's pixel is over the threshold both times
    low = np.zeros((22, 26), np.int64)
    low[PLATEAU[1]:PLATEAU[3] + 1, PLATEAU[0]:PLATEAU[2] + 1] = 3000
    low[SPIKE[1], SPIKE[0]] = 5000
    cs.append(case("first_flag", low, 100, 8, extra=0, radius=[1, 3]))
    # dh_max reached before the last step: 230, 230, 260, then 320 cut to 300.  A 12 x 12 plateau of 310, which only the
    # 17 x 17 window of the last step removes, is flagged because of the cut
    low = np.zeros((32, 40), np.int64)
    low[CAP_PLATEAU[1]:CAP_PLATEAU[3] + 1, CAP_PLATEAU[0]:CAP_PLATEAU[2] + 1] = 310
    cs.append(case("cap", low, 100, 9, radius=[1, 2, 4, 8], dh_max=300))
    cs.append(case("sixteen", relief(40, 32, 10), 100, 10, radius=list(range(1, 17))))
    # z on both sides of 0, and the two ends of the range
    low = relief(32, 24, 11) - 3000
    low[3, 4], low[20, 27] = -Z_LIMIT, Z_LIMIT
    cs.append(case("negative", low, 100, 11, radius=[1, 2, 4]))
    cs.append(scene_case(100))
    cs.append(scene_case(200))
    return cs


CASES = build()
BY_NAME = {c["name"]: c for c in CASES}


def args(c):
    return c["xyz"], c["extent"], c["params"]


def big():
    """about 600 000 points over the lattice of `odd`: more than one sweep of both passes over the points"""
    low = relief(131, 67, 5, boxes=6)
    c = case("big", low, 100, 12, extra=-(-BIG_POINTS // low.size), radius=[1, 3, 7, 20])
    return c
