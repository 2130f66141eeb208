"""Clouds for the roof tests and tests/tools/roof_bench.py."""
import numpy as np

from buildingsegment_amd import synth

EAVES, RIDGE = 3000, 4500  # of the gabled house
GABLE_X, GABLE_Y = (0, 8000), (0, 6000)  # its footprint before the shift to the origin (the ridge runs along y)
MARGIN = 3000  # ground sheet around everything: the shift to the origin moves every coordinate by this much


def _grid(a0, a1, b0, b1, spacing):
    a, b = np.meshgrid(np.arange(a0, a1 + 1, spacing, dtype=np.int64), np.arange(b0, b1 + 1, spacing, dtype=np.int64),
                       indexing="ij")
    return a.ravel(), b.ravel()


def _flat(x0, x1, y0, y1, z, spacing=50):
    x, y = _grid(x0, x1, y0, y1, spacing)
    return np.stack([x, y, np.full(x.size, z, np.int64)], 1)


def gabled(seed=41):
    """A gabled house (8 m x 6 m, eaves at 3 m, ridge at 4.5 m along y, four walls), a flat-roofed house at 3.5 m, an
    L-shaped flat roof at 4 m whose two arms are sampled as separate sheets with a 50 mm seam between them, and a
    200 mm ground sheet with a 3 m margin.  Jittered, shuffled and shifted to the origin; about 0.1 M points."""
    (gx0, gx1), (gy0, gy1) = GABLE_X, GABLE_Y
    mid = (gx0 + gx1) // 2
    slope = (RIDGE - EAVES) / (mid - gx0)
    x, y = _grid(gx0, mid, gy0, gy1, 50)
    west = np.stack([x, y, np.rint(EAVES + slope * (x - gx0)).astype(np.int64)], 1)
    x, y = _grid(mid + 50, gx1, gy0, gy1, 50)
    east = np.stack([x, y, np.rint(EAVES + slope * (gx1 - x)).astype(np.int64)], 1)
    walls = []
    for yw in (gy0, gy1):
        x, z = _grid(gx0, gx1, 0, EAVES - 50, 50)
        walls.append(np.stack([x, np.full(x.size, yw, np.int64), z], 1))
    for xw in (gx0, gx1):
        y, z = _grid(gy0, gy1, 0, EAVES - 50, 50)
        walls.append(np.stack([np.full(y.size, xw, np.int64), y, z], 1))
    flat = _flat(14000, 20000, 0, 6000, 3500)
    arm1 = _flat(0, 8000, 12000, 15000, 4000)
    arm2 = _flat(25, 3000, 15050, 20000, 4000)
    every = np.concatenate([west, east] + walls + [flat, arm1, arm2])
    mn, mx = every.min(0), every.max(0)
    ground = _flat(mn[0] - MARGIN, mx[0] + MARGIN, mn[1] - MARGIN, mx[1] + MARGIN, 0, 200)
    under = np.zeros(len(ground), bool)  # (a scanner above the roofs does not see the ground beneath them)
    for x0, x1, y0, y1 in ((gx0, gx1, gy0, gy1), (14000, 20000, 0, 6000), (0, 8000, 12000, 15000), (0, 3000, 15000, 20000)):
        under |= (ground[:, 0] >= x0) & (ground[:, 0] <= x1) & (ground[:, 1] >= y0) & (ground[:, 1] <= y1)
    pts = np.concatenate([every, ground[~under]])
    rng = np.random.default_rng(seed)
    pts[:, :2] += rng.integers(-10, 11, (len(pts), 2))
    pts[:, 2] += rng.integers(-5, 6, len(pts))
    pts = pts[synth.permutation(seed, 99, len(pts))]
    return synth.shift_to_origin(pts)


def gable_pixels(bin=100):
    """(row, columns): the pixel row through the middle of the gabled house and its columns from eaves to eaves
    (whole pixels inside the footprint), in the shifted cloud."""
    row = (MARGIN + 10 + (GABLE_Y[0] + GABLE_Y[1]) // 2) // bin
    x0, x1 = MARGIN + 10 + GABLE_X[0], MARGIN + 10 + GABLE_X[1]
    return row, np.arange(x0 // bin + 1, x1 // bin)
