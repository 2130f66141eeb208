"""Clouds for the building tests and tests/tools/building_bench.py."""
import numpy as np

from buildingsegment_amd import synth


def _sheet(x0, x1, y0, y1, z, spacing):
    x, y = np.meshgrid(np.arange(x0, x1 + 1, spacing, dtype=np.int64), np.arange(y0, y1 + 1, spacing, dtype=np.int64),
                       indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, z, np.int64)], 1)


def composed(seed=33):
    """Twelve box buildings on a 9 m grid, a 200 mm ground sheet with a 3 m margin under everything, a 20 m square
    ring roof at 9 m around a 10 m courtyard (whose floor is the sparse ground sheet: enclosed pixels that are not
    foreground), and a low 4 m slab at 1.2 m beside the ring (a plane of its own that lies in no building).
    Shuffled and shifted to the origin; about 0.78 M points.  After the shuffle the slab's centre point is moved to
    index 0: the seed scan then commits the slab first, before any failed seed has left orphans that would carry
    its id into a building."""
    box = synth.boxes(n_boxes=12, edge_lo=80, edge_hi=120, pitch=9000, shuffle=False).astype(np.int64)
    ry = int(box[:, 1].max()) + 6000  # the ring lies beyond the boxes in y
    roof = _sheet(0, 20000, ry, ry + 20000, 9000, 50)
    inner = (roof[:, 0] > 5000) & (roof[:, 0] < 15000) & (roof[:, 1] > ry + 5000) & (roof[:, 1] < ry + 15000)
    roof = roof[~inner]
    slab = _sheet(25000, 29000, ry + 5000, ry + 9000, 1200, 50)
    every = np.concatenate([box, roof, slab])
    mn, mx = every.min(0), every.max(0)
    ground = _sheet(mn[0] - 3000, mx[0] + 3000, mn[1] - 3000, mx[1] + 3000, 0, 200)
    pts = np.concatenate([every, ground])
    rng = np.random.default_rng(seed)
    pts[:, :2] += rng.integers(-10, 11, (len(pts), 2))  # in-plane jitter of the sheets
    pts[:, 2] += rng.integers(-5, 6, len(pts))
    centre = len(box) + len(roof) + len(slab) // 2
    perm = synth.permutation(seed, 99, len(pts))
    at = int(np.flatnonzero(perm == centre)[0])
    perm[0], perm[at] = perm[at], perm[0]
    pts = pts[perm]
    return synth.shift_to_origin(pts)
