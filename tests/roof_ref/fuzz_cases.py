"""The 40 seeded cases of the roof fuzz (tests/test_gpu_roofs.py runs them on the device, tests/test_roofs_cpu.py
asserts on the restatement alone that they reach every regime) and the regime detectors."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "building_ref"))
import building_ref as bref  # noqa: E402
import roof_ref as rr  # noqa: E402

N_CASES = 40
FIG_CAP = 2048   # planes whose figures the device reduces in LDS (bs_roof.hip)
FILL_GROUP = 8   # fill rounds the device launches per host round trip (bs_roof.hip)


def _mask(rng, h, w):
    m = np.zeros((h, w), bool)
    for _ in range(int(rng.integers(1, 7))):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        m[y0:y0 + int(rng.integers(1, h // 2 + 2)), x0:x0 + int(rng.integers(1, w // 2 + 2))] = True
    if rng.random() < 0.5:
        m &= rng.random((h, w)) < 0.93  # holes: what a building encloses belongs to it
    if rng.random() < 0.3:  # a long one-pixel corridor: many fill rounds
        m[h // 2, :] = True
    return m


def fuzz_case(seed):
    """dict(xyz, bmap, plane_idx, n_planes, home, normal, center, bin, ground_th, min_votes)"""
    rng = np.random.default_rng(1000 + seed)
    if seed % 10 == 0:  # a plain case: one building, one flat plane, every pixel seeded, whole waves
        h, w, bin_ = 8 + seed // 10, 16, 10
        ys, xs = np.mgrid[0:h, 0:w]
        xyz = np.stack([xs.ravel() * bin_ + 3, ys.ravel() * bin_ + 4, 2000 + (np.arange(h * w) % 7) * 10], 1)
        xyz = np.concatenate([xyz, xyz])[:(2 * h * w) // 64 * 64]
        xyz[:, 2] -= 30 * (np.arange(len(xyz)) % 2)
        return dict(xyz=xyz.astype(np.int32), bmap=np.zeros((h, w), np.int32), plane_idx=np.ones(len(xyz), np.int32),
                    n_planes=1, home=np.zeros(1, np.int32), normal=np.array([[0.0, 0.0, 1.0]]),
                    center=np.array([[40, 40, 2010]], np.int32), bin=bin_, ground_th=0.0, min_votes=1)
    h, w = (int(rng.integers(1, 151)) for _ in range(2))
    if seed % 10 == 1:
        h, w = 1, int(rng.integers(60, 151))
    bin_ = int(rng.choice([1, 7, 37, 100]))
    mask = _mask(rng, h, w)
    b = bref.building_map(mask)
    bmap, nb = b.map.copy(), b.n_buildings
    if seed % 3 == 0 and nb:  # hand-edited adjacency: the right part of building 0 becomes a building of its own
        ys, xs = np.nonzero(bmap == 0)
        cut = (xs.min() + xs.max() + 1) // 2
        if (xs >= cut).any() and (xs < cut).any():
            bmap[ys[xs >= cut], xs[xs >= cut]] = nb
            nb += 1
    n = int(rng.choice([1, 17, 63, 64, 65, 640, 3000, 12345, 30000], p=[.05, .05, .05, .05, .05, .15, .2, .2, .2]))
    n_planes = int(rng.choice([1, 3, 12, 2500]))
    ground_th = float(rng.choice([0.0, 1000.0, 1500.5]))
    # where the points fall: everywhere, or only in a corner of one building's box (the fill then has far to go)
    x0 = y0 = 0
    x1, y1 = w * bin_, h * bin_
    if nb and rng.random() < 0.6:
        ys, xs = np.nonzero(bmap == int(rng.integers(0, nb)))
        x0, y0 = int(xs.min()) * bin_, int(ys.min()) * bin_
        x1 = x0 + max(int((xs.max() + 1 - xs.min()) * bin_ * float(rng.choice([0.05, 0.2, 1.0]))), 1)
        y1 = y0 + max(int((ys.max() + 1 - ys.min()) * bin_ * float(rng.choice([0.1, 1.0]))), 1)
    xyz = np.stack([rng.integers(x0, x1, n), rng.integers(y0, y1, n), rng.integers(-500, 6000, n)], 1).astype(np.int32)
    if rng.random() < 0.4:  # several points per pixel: real counts, ties
        xyz[:, :2] = xyz[rng.integers(0, max(n // 8, 1), n), :2]
    if ground_th == 1000.0:
        xyz[rng.random(n) < 0.1, 2] = 1000
    home = rng.integers(-1, max(nb, 1), n_planes).astype(np.int32) if nb else np.full(n_planes, -1, np.int32)
    # labels: mostly a plane that is at home in the building under the point, so that points count
    under = bmap[xyz[:, 1] // bin_, xyz[:, 0] // bin_]
    plane = rng.integers(-1, n_planes + 2, n).astype(np.int32)
    at_home = np.zeros(n, np.int32)
    for k in range(n):
        cand = np.flatnonzero(home == under[k]) if under[k] >= 0 else []
        at_home[k] = (cand[rng.integers(0, min(len(cand), 3))] + 1) if len(cand) else 0
    if n_planes == 2500:  # half of those in a plane above the LDS tables, where there is one
        hi = np.array([(np.flatnonzero(home[2060:] == u)[:1] + 2061).sum() if u >= 0 else 0 for u in under], np.int32)
        at_home = np.where((hi > 0) & (rng.random(n) < 0.5), hi, at_home)
    plane = np.where((rng.random(n) < 0.7) & (at_home > 0), at_home, plane).astype(np.int32)
    if rng.random() < 0.5:
        plane[plane == n_planes + 1] = -1
    normal = rng.normal(size=(n_planes, 3))
    normal[:, 2] = np.abs(normal[:, 2]) + 0.2
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    flat = rng.random(n_planes) < 0.3
    normal[flat] = [0.0, 0.0, 1.0]
    odd = rng.random(n_planes) < 0.1
    normal[odd, 2] = rng.choice([0.0, -0.3, np.nan], int(odd.sum()))
    center = np.stack([rng.integers(0, w * bin_, n_planes), rng.integers(0, h * bin_, n_planes),
                       rng.integers(1000, 5000, n_planes)], 1).astype(np.int32)
    return dict(xyz=xyz, bmap=bmap.astype(np.int32), plane_idx=plane, n_planes=n_planes, home=home, normal=normal,
                center=center, bin=bin_, ground_th=ground_th, min_votes=int(rng.choice([1, 2, 5], p=[.6, .25, .15])))


def run_ref(c):
    return rr.roofs(c["xyz"], c["bmap"], c["plane_idx"], c["n_planes"], c["home"], c["normal"], c["center"], c["bin"],
                    c["ground_th"], c["min_votes"])


def regimes(c, r):
    """The set of regimes case c (with its restatement result r) reaches."""
    out = set()
    n, npl, bmap = len(c["xyz"]), c["n_planes"], c["bmap"]
    ok, pix, plane = r.counting, r.pixel, c["plane_idx"].astype(np.int64)
    # the count of every (pixel, plane) pair, the top count of every pixel and how many planes share it
    pair, cnt = np.unique(pix[ok] * (npl + 2) + plane[ok], return_counts=True)
    ppix = pair // (npl + 2)
    top = np.zeros(bmap.size, np.int64)
    np.maximum.at(top, ppix, cnt)
    sharing = np.bincount(ppix[cnt == top[ppix]], minlength=bmap.size)
    if ((sharing > 1) & (top >= c["min_votes"])).any():
        out.add("tie")
    if (top[np.unique(ppix)] < c["min_votes"]).any():
        out.add("min_votes")
    if (c["xyz"][:, 2].astype(np.float64) == c["ground_th"]).any():
        out.add("z_equals_ground_th")
    if (plane == npl + 1).any():
        out.add("label_n_planes_plus_1")
    if r.fill_rounds >= 5:
        out.add("fill_5_rounds")
    if r.fill_rounds > FILL_GROUP:
        out.add("threshold_fill_group")
    roof = r.seed_roof
    while True:  # two seeds reaching a pixel in the same round: its labelled neighbours disagree when it is filled
        lo = np.full(roof.shape, rr.I32_MAX, np.int64)
        hi = np.zeros(roof.shape, np.int64)
        for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)):
            nr, nm = rr._shift(roof, dy, dx, 0), rr._shift(bmap, dy, dx, -2)
            good = (nm == bmap) & (nr > 0)
            lo, hi = np.minimum(lo, np.where(good, nr, rr.I32_MAX)), np.maximum(hi, np.where(good, nr, 0))
        upd = (roof == 0) & (hi > 0)
        if (upd & (lo != hi)).any():
            out.add("two_seeds_one_round")
        if not upd.any():
            break
        roof = np.where(upd, lo, roof).astype(np.int32)
    if (r.roof == 0).any():
        out.add("unroofed_building")
    ys, xs = np.nonzero(r.roof > 0)
    if len(ys):
        s = r.roof[ys, xs].astype(np.int64) - 1
        nrm, ctr = np.asarray(c["normal"], np.float64)[s], np.asarray(c["center"], np.float64)[s]
        with np.errstate(all="ignore"):
            z = ctr[:, 2] - (nrm[:, 0] * (xs * c["bin"] + c["bin"] // 2 - ctr[:, 0]) +
                             nrm[:, 1] * (ys * c["bin"] + c["bin"] // 2 - ctr[:, 1])) / nrm[:, 2]
        if (z < r.z_min[s]).any():
            out.add("lower_clamp")
        if (z > r.z_max[s]).any():
            out.add("upper_clamp")
    if n < 64:
        out.add("fewer_than_64_points")
    if n % 64:
        out.add("partial_last_wave")
    if (r.n_support[FIG_CAP:] > 0).any() and (r.pixels[FIG_CAP:] > 0).any():
        out.add("threshold_fig_cap")
    return out


ALL_REGIMES = ("tie", "min_votes", "z_equals_ground_th", "label_n_planes_plus_1", "fill_5_rounds", "two_seeds_one_round",
               "unroofed_building", "lower_clamp", "upper_clamp", "fewer_than_64_points", "partial_last_wave",
               "threshold_fig_cap", "threshold_fill_group")
