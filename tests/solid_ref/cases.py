"""Seeded cases for the solids (include/bs_api.h, "solids"): small ones for brute force against the restatement, the
fuzz cases of the device suite, and `regimes`: which rows of the threshold table ("Solids") a case reaches,
worked out from its inputs alone (the tops and a walk over the pixels; no mesh is built)."""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import solid_ref as sr  # noqa: E402

FIG_CAP = 1024  # of bs_solid.hip: buildings from this id on take the global-atomic path of the figures
N_SMALL, N_FUZZ = 60, 40
KEYS = ("bmap", "roof", "n_buildings", "normal", "center", "z_min", "z_max", "bin", "base_z", "flat")
# every row of the threshold table that a case of at most 96 x 96 can reach (the grid strides and the scan's tiles need
# a million pixels: tests/test_gpu_solids.py::test_large_image_with_blobs)
REGIMES = ("wall_triangle", "wall_quad", "wall_crossing", "wall_mid_up", "wall_mid_down", "wall_8", "wall_inner",
           "wall_outer", "image_border", "other_building", "unroofed", "top_at_base", "below_base", "corner_8",
           "corner_5_heights", "building_lds", "building_global", "wave_uniform", "wave_mixed", "no_planes", "no_pixels",
           "nan_plane", "nz_not_positive", "clamp_min", "clamp_max")


def make(bmap, roof, n_buildings, normal, center, z_min, z_max, bin, base_z, flat):
    bmap = np.asarray(bmap, np.int32)
    roof = np.where(bmap < 0, -1, np.asarray(roof, np.int32)).astype(np.int32)
    return dict(bmap=bmap, roof=roof, n_buildings=int(n_buildings), normal=np.asarray(normal, np.float64).reshape(-1, 3),
                center=np.asarray(center, np.int32).reshape(-1, 3), z_min=np.asarray(z_min, np.int32).reshape(-1),
                z_max=np.asarray(z_max, np.int32).reshape(-1), bin=int(bin), base_z=int(base_z),
                flat=np.asarray(flat, np.int32).reshape(-1))


def run_ref(c):
    return sr.solids(*[c[k] for k in KEYS])


def _planes(rng, n, w, h, bin, zlo, zhi, slope):
    normal = np.stack([rng.normal(0, slope, n), rng.normal(0, slope, n), np.ones(n)], 1)
    center = np.stack([rng.integers(0, w * bin + 1, n), rng.integers(0, h * bin + 1, n), rng.integers(zlo, zhi + 1, n)], 1)
    return normal, center


def _patches(rng, h, w, n_values, size):
    """an image of patches of about size x size with values 0 .. n_values - 1"""
    gy, gx = -(-h // size) + 1, -(-w // size) + 1
    grid = rng.integers(0, n_values, (gy, gx))
    oy, ox = rng.integers(0, size, 2)
    yy, xx = np.mgrid[0:h, 0:w]
    return grid[(yy + oy) // size, (xx + ox) // size]


def small_case(seed):
    """at most 12 x 12: adjacent buildings, unroofed pixels, tops equal to base_z and heights from a 3-value range"""
    rng = np.random.default_rng(1000 + seed)
    h, w = (int(v) for v in rng.integers(1, 13, 2))
    nb = int(rng.integers(1, 5))
    bin = int(rng.choice([1, 7, 10]))
    base = int(rng.integers(-1, 2))
    spread = [1, 3, 1000][seed % 3]
    bmap = rng.integers(-1 if seed % 4 else 0, nb, (h, w))
    npl = int(rng.integers(0, 5)) if seed % 5 else 0
    roof = rng.integers(0, npl + 1, (h, w))
    if spread <= 3:  # flat planes at a few heights: coincidences everywhere
        normal = np.tile([0.0, 0.0, 1.0], (npl, 1))
        center = np.stack([np.zeros(npl), np.zeros(npl), base + rng.integers(0, spread, npl)], 1)
    else:
        normal, center = _planes(rng, npl, w, h, bin, base + 490, base + 510, 2.0)  # close together: the planes cross
    return make(bmap, roof, nb, normal, center, np.full(npl, base - 2), np.full(npl, base + spread), bin, base,
                base + rng.integers(-1, spread, nb))


def fuzz_case(seed):
    """the cases of the device suite: at most 96 x 96, eight kinds"""
    rng = np.random.default_rng(7000 + seed)
    kind = seed % 8
    h, w = (int(v) for v in rng.integers(20, 97, 2))
    bin, base = int(rng.choice([5, 10, 25])), int(rng.integers(-50, 50))
    if kind == 0:  # small and dense, heights from a 3-value range
        c = small_case(500 + seed)
        return c
    if kind == 1:  # buildings as patches with gaps, sloped planes in patches
        nb, npl = 12, 6
        bmap = _patches(rng, h, w, nb + 4, 9) - 4
        roof = _patches(rng, h, w, npl + 1, 5)
        normal, center = _planes(rng, npl, w, h, bin, base + 2000, base + 4000, 0.3)
        return make(bmap, roof, nb, normal, center, np.full(npl, base + 1500), np.full(npl, base + 5000), bin, base,
                    base + rng.integers(0, 3000, nb))
    if kind == 2:  # more buildings than the figure tables hold: every pixel of a checkerboard its own building
        h, w = max(h, 50), max(w, 50)
        yy, xx = np.mgrid[0:h, 0:w]
        on = (yy + xx) % 2 == 0
        bmap = np.where(on, np.cumsum(on.ravel()).reshape(h, w) - 1, -1)
        nb = int(on.sum())
        return make(bmap, np.zeros((h, w)), nb, np.zeros((0, 3)), np.zeros((0, 3)), [], [], bin, base,
                    base + rng.integers(0, 4, nb))
    if kind == 3:  # a steep plane of its own choice on every pixel: walls with vertices in between, crossing walls
        nb, npl = 3, 8
        bmap = _patches(rng, h, w, nb + 1, 14) - 1
        roof = rng.integers(1, npl + 1, (h, w))
        normal, center = _planes(rng, npl, w, h, bin, base, base + 500, 3.0)
        return make(bmap, roof, nb, normal, center, np.full(npl, base - 100), np.full(npl, base + 600), bin, base,
                    np.full(nb, base + 100))
    if kind == 4:  # no plane at all: everything is flat, some buildings at base_z
        nb = 9
        bmap = _patches(rng, h, w, nb + 2, 6) - 2
        flat = base + rng.integers(-2, 3, nb) * 100
        return make(bmap, np.zeros((h, w)), nb, np.zeros((0, 3)), np.zeros((0, 3)), [], [], bin, base, flat)
    if kind == 5:  # planes the clamps decide: NaN, nz <= 0, far away, below base_z
        nb, npl = 4, 7
        bmap = _patches(rng, h, w, nb + 1, 11) - 1
        roof = _patches(rng, h, w, npl + 1, 4)
        normal, center = _planes(rng, npl, w, h, bin, base - 300, base + 300, 1.0)
        normal[0] = [0.3, np.nan, 1.0]
        normal[1] = [0.2, 0.1, 0.0]
        normal[2] = [0.2, 0.1, -0.7]
        normal[3] = [50.0, -40.0, 0.01]
        zmin, zmax = base + rng.integers(-400, 100, npl), base + rng.integers(100, 500, npl)
        zmin[4], zmax[4] = sr.I32_MAX, sr.I32_MIN  # a plane without a supporting point
        return make(bmap, roof, nb, normal, center, zmin, zmax, bin, base, base + rng.integers(-100, 300, nb))
    if kind == 6:  # one wide building under two sloped planes: whole waves inside it
        w = max(w, 70)
        bmap = np.zeros((h, w))
        bmap[:, : int(rng.integers(0, 3))] = -1
        roof = 1 + (np.arange(w)[None, :] >= w // 2) * np.ones((h, 1), np.int64)
        normal = np.array([[-0.4, 0.0, 0.9], [0.4, 0.0, 0.9]])
        center = np.array([[w * bin // 4, 0, base + 3000], [3 * w * bin // 4, 0, base + 3000]])
        return make(bmap, roof, 1, normal, center, [base + 2000] * 2, [base + 5000] * 2, bin, base, [base + 2500])
    # kind 7: many buildings in single pixels next to each other (corners with four buildings), or no pixel at all
    if seed % 16 == 15:
        return make(np.full((h, w), -1), np.full((h, w), -1), 3, np.zeros((0, 3)), np.zeros((0, 3)), [], [], bin, base,
                    [base, base + 1, base + 2])
    nb = 40
    bmap = rng.integers(-1, nb, (h, w))
    npl = 3
    normal, center = _planes(rng, npl, w, h, bin, base + 100, base + 200, 0.5)
    return make(bmap, rng.integers(0, npl + 1, (h, w)), nb, normal, center, np.full(npl, base), np.full(npl, base + 300),
                bin, base, base + rng.integers(0, 200, nb))


def blob_case(w, h, seed, size=9, nb=12):
    """buildings as patches of about size x size with gaps, sloped planes in smaller patches, some pixels unroofed"""
    rng = np.random.default_rng(9000 + seed)
    npl, bin, base = 6, 10, 100
    bmap = _patches(rng, h, w, nb + max(nb // 3, 1), size) - max(nb // 3, 1)
    roof = _patches(rng, h, w, npl + 1, max(size // 2, 2))
    normal, center = _planes(rng, npl, w, h, bin, base + 2000, base + 4000, 0.3)
    return make(bmap, roof, nb, normal, center, np.full(npl, base + 1500), np.full(npl, base + 5000), bin, base,
                base + rng.integers(0, 3000, nb))


def grid_of_buildings(nb, seed=0):
    """nb single-pixel buildings on a grid with gaps (every second pixel of every second row), flat tops"""
    rng = np.random.default_rng(seed)
    per_row = int(np.ceil(np.sqrt(nb)))
    rows = -(-nb // per_row)
    bmap = np.full((2 * rows, 2 * per_row), -1)
    ids = np.arange(rows * per_row).reshape(rows, per_row)
    bmap[::2, ::2] = np.where(ids < nb, ids, -1)
    return make(bmap, np.zeros(bmap.shape), nb, np.zeros((0, 3)), np.zeros((0, 3)), [], [], 10, 0, rng.integers(0, 50, nb))


def regimes(c):
    """the rows of REGIMES this case reaches, from its inputs"""
    bmap, roof, base, nb = c["bmap"].astype(np.int64), c["roof"].astype(np.int64), c["base_z"], c["n_buildings"]
    h, w = bmap.shape
    out = set()
    inb = bmap >= 0
    if not inb.any():
        return {"no_pixels"} | ({"no_planes"} if len(c["z_min"]) == 0 else set())
    top = sr.tops(*[c[k] for k in KEYS if k != "n_buildings"]).astype(np.int64)
    if len(c["z_min"]) == 0:
        out.add("no_planes")
    if (inb & (roof <= 0)).any():
        out.add("unroofed")
    if (top[inb] == base).all(1).any():
        out.add("top_at_base")
    if (bmap[inb] < FIG_CAP).any():
        out.add("building_lds")
    if (bmap >= FIG_CAP).any():
        out.add("building_global")
    flat = np.where(inb, bmap, -1).ravel()
    flat = np.concatenate([flat, np.full(-len(flat) % 64, -1)]).reshape(-1, 64)
    uni = (flat == flat[:, :1]).all(1)
    if (uni & (flat[:, 0] >= 0)).any():
        out.add("wave_uniform")
    if (~uni).any():
        out.add("wave_mixed")
    # the unclamped heights of the roofed pixels: which clamp decided, and whether base_z did
    ys, xs = np.nonzero(inb & (roof > 0))
    if len(ys):
        s = roof[ys, xs] - 1
        n, ce = c["normal"][s], c["center"][s].astype(np.float64)
        if np.isnan(n).any():
            out.add("nan_plane")
        if (n[:, 2] <= 0).any():
            out.add("nz_not_positive")
        with np.errstate(all="ignore"):
            for k in range(4):
                z = ce[:, 2] - (n[:, 0] * ((xs + (k & 1)) * c["bin"] - ce[:, 0]) + n[:, 1] * ((ys + (k >> 1)) * c["bin"] - ce[:, 1])) / n[:, 2]
                lo, hi = c["z_min"][s].astype(np.float64), c["z_max"][s].astype(np.float64)
                if (~(z >= lo)).any():
                    out.add("clamp_min")
                z = np.where(~(z >= lo), lo, z)
                if (z > hi).any():
                    out.add("clamp_max")
                z = np.where(z > hi, hi, z)
                if (z.astype(np.int64) < base).any():
                    out.add("below_base")
    # corners and walls, pixel by pixel
    heights = {}
    for y, x in zip(*np.nonzero(inb)):
        for k in range(4):
            heights.setdefault((y + (k >> 1), x + (k & 1)), {}).setdefault(int(bmap[y, x]), {base}).add(int(top[y, x, k]))
    for per in heights.values():
        if sum(len(v) for v in per.values()) == 8:
            out.add("corner_8")
        if max(len(v) for v in per.values()) == 5:
            out.add("corner_5_heights")
    for y, x in zip(*np.nonzero(inb)):
        b = int(bmap[y, x])
        for d, (ks, ke, (dx, dy), ns, ne) in enumerate(sr.WALLS):
            nx, ny = x + dx, y + dy
            inside = 0 <= nx < w and 0 <= ny < h
            same = inside and bmap[ny, nx] == b
            if same and d in (0, 3):
                continue
            a_s, a_e = int(top[y, x, ks]), int(top[y, x, ke])
            b_s, b_e = (int(top[ny, nx, ns]), int(top[ny, nx, ne])) if same else (base, base)
            if (a_s, a_e) == (b_s, b_e):
                continue
            out.add("wall_inner" if same else "wall_outer")
            if not inside:
                out.add("image_border")
            elif not same and bmap[ny, nx] >= 0:
                out.add("other_building")
            if (a_s == b_s) != (a_e == b_e):
                out.add("wall_triangle")
            elif (a_s - b_s) * (a_e - b_e) < 0:
                out.add("wall_crossing")
            else:
                out.add("wall_quad")
            mids = 0
            for (Y, X), z0, z1 in (((y + (ks >> 1), x + (ks & 1)), a_s, b_s), ((y + (ke >> 1), x + (ke & 1)), b_e, a_e)):
                between = sum(min(z0, z1) < z < max(z0, z1) for z in heights[Y, X][b])
                mids += between
                if between:
                    out.add("wall_mid_up" if z0 < z1 else "wall_mid_down")
            if 4 + mids == 8:
                out.add("wall_8")
    assert out <= set(REGIMES), out - set(REGIMES)
    return out


def _flat_planes(zs):
    """flat planes at the heights zs (plane p is zs[p - 1]) with clamps that never decide"""
    n = len(zs)
    return (np.tile([0.0, 0.0, 1.0], (n, 1)), np.stack([np.zeros(n), np.zeros(n), np.asarray(zs)], 1), np.full(n, -10 ** 6),
            np.full(n, 10 ** 6))


def _two_pixels(cz, ny):
    """pixels (0, 0) and (1, 0) of one building, bin 10: plane 1 flat at 100, plane 2 z = cz - ny * Y along the shared edge"""
    normal = np.array([[0.0, 0.0, 1.0], [0.0, ny, 1.0]])
    center = np.array([[0, 0, 100], [0, 0, cz]])
    return make([[0, 0]], [[1, 2]], 1, normal, center, [-10 ** 6] * 2, [10 ** 6] * 2, 10, 0, [0])


def named_shapes():
    """name -> case: the shapes the tests name"""
    out = {}
    out["one_pixel"] = make([[0]], [[0]], 1, *_flat_planes([]), 10, 0, [50])
    out["one_pixel_at_base"] = make([[0]], [[0]], 1, *_flat_planes([]), 10, 50, [50])
    out["two_pixels_triangle"] = _two_pixels(100, -1.0)  # 100 and 110 against 100 and 100
    out["two_pixels_quad"] = _two_pixels(120, 0.0)       # 120 and 120
    out["two_pixels_crossing"] = _two_pixels(95, -1.0)   # 95 and 105
    out["corner_four_heights"] = make([[0, 0], [0, 0]], [[1, 4], [3, 2]], 1, *_flat_planes([10, 20, 30, 40]), 10, 0, [0])
    yy, xx = np.mgrid[0:6, 0:7]
    out["checkerboard"] = make(np.where((yy + xx) % 2 == 0, 0, -1), 1 + yy % 2, 1, *_flat_planes([30, 60]), 5, -4, [0])
    out["two_buildings"] = make([[0, 0, 1, 1], [0, 0, 1, 1]], [[1, 1, 2, 2], [1, 1, 0, 2]], 2, *_flat_planes([70, 70]), 10, 0,
                                [70, 40])
    out["borders"] = make([[-1, 0, -1], [0, -1, 0], [-1, 0, -1]], np.zeros((3, 3)), 1, *_flat_planes([]), 10, 0, [25])
    return out

