"""Clouds and seeded cases for the plane-fit tests and tests/tools/fit_bench.py."""
import numpy as np

LIM = 2 ** 23 - 1  # the largest coordinate of the domain
# what the passes of bs_fit.hip switch on ("Plane fit"): planes above FIT_CAP leave the LDS tables, a wave
# is 64 consecutive points, a workgroup takes TILE consecutive points per trip and GRID workgroups stride over the cloud
FIT_CAP, WAVE, TILE, GRID = 3072, 64, 4096, 256
N_CASES = 46

SHEET_X0, SHEET_Y0 = 200_000, 150_000


def sheet_z(x, y):
    """the generating plane of tilted_sheet, f64"""
    return 5000.0 + 0.3 * (np.asarray(x, np.float64) - SHEET_X0) + 0.1 * (np.asarray(y, np.float64) - SHEET_Y0)


def tilted_sheet(seed=0):
    """The scene the plane fit exists for: a 300 x 300 grid at 50 mm far from the origin (x from 200 000, y from
    150 000) on the plane sheet_z, +-10 mm of integer noise in z; 90 000 points, all coordinates positive, unshifted."""
    g = np.arange(300, dtype=np.int64) * 50
    x, y = np.meshgrid(SHEET_X0 + g, SHEET_Y0 + g, indexing="ij")
    x, y = x.ravel(), y.ravel()
    z = np.rint(sheet_z(x, y)).astype(np.int64) + np.random.default_rng(seed).integers(-10, 11, x.size)
    return np.stack([x, y, z], 1).astype(np.int32)


def patches(rng, n, n_planes, spread=4000, noise=5, junk=0.1, big_from=0):
    """n points on n_planes noisy tilted patches anywhere in the domain, labels 1 .. n_planes drawn at random, a share
    (half of the points on up to 8 big planes with ids above big_from, so that whole waves of one label occur), a share
    `junk` of them replaced by -1, 0 and n_planes + 1 (ignored labels)"""
    base = rng.integers(-(LIM - 4 * spread), LIM - 4 * spread + 1, (n_planes, 3))
    slope = rng.uniform(-1.5, 1.5, (n_planes, 2))
    lab = rng.integers(0, n_planes, n)
    big = rng.integers(min(big_from, n_planes - 1), n_planes, min(8, n_planes))
    lab = np.where(rng.random(n) < 0.5, big[rng.integers(0, len(big), n)], lab)
    uv = rng.integers(-spread, spread + 1, (n, 2))
    z = np.rint(slope[lab, 0] * uv[:, 0] + slope[lab, 1] * uv[:, 1]).astype(np.int64) + rng.integers(-noise, noise + 1, n)
    xyz = base[lab] + np.stack([uv[:, 0], uv[:, 1], z], 1)
    vertical = rng.random(n_planes) < 0.2  # every fifth patch is a wall: x and z change places
    sw = vertical[lab]
    xyz[sw] = (base[lab] + np.stack([z, uv[:, 1], uv[:, 0]], 1))[sw]
    plane = (lab + 1).astype(np.int32)
    j = rng.random(n) < junk
    plane[j] = rng.choice(np.array([-1, 0, n_planes + 1], np.int32), int(j.sum()))
    return np.clip(xyz, -LIM, LIM).astype(np.int32), plane


def layout(rng, xyz, plane, kind):
    """contiguous: by plane, the ignored labels first (whole waves of one label); random: a permutation (every lane
    another plane); mixed: the first half contiguous, the rest permuted"""
    n = len(plane)
    by = np.argsort(plane, kind="stable")
    if kind == "contiguous":
        o = by
    elif kind == "random":
        o = rng.permutation(n)
    else:
        o = np.concatenate([by[: n // 2], rng.permutation(by[n // 2:])])
    return np.ascontiguousarray(xyz[o]), np.ascontiguousarray(plane[o])


def fuzz_case(seed):
    """cases 0 .. 39: n from 1 to 30 000 and 1 to 2 500 planes in the three layouts; 40 .. 45: more planes than the LDS
    tables hold (the fuzz has to reach the global-atomic regimes too).  Every fourth case carries a plane too large
    for the exact sums (status 2) where it has the points for one."""
    rng = np.random.default_rng(7000 + seed)
    kind = ("contiguous", "random", "mixed")[seed % 3]
    if seed < 40:
        n = int(np.exp(rng.uniform(0, np.log(30_000)))) if seed % 5 else (1, 2, 3, 64, 30_000, 4097, 4096, 65)[seed // 5]
        n_planes = int(np.exp(rng.uniform(0, np.log(2500)))) if seed % 7 else (1, 2500, 2, 1000, 64, 300)[seed // 7]
    else:
        n, n_planes = int(rng.integers(15_000, 30_001)), int(rng.integers(FIT_CAP + 1, 6001))
    xyz, plane = patches(rng, n, n_planes, spread=int(rng.choice([0, 3, 500, 4000, 100_000])), noise=int(rng.choice([0, 5, 40])),
                         big_from=FIT_CAP if seed >= 40 else 0)
    if seed % 4 == 0 and n >= 24_000:
        # 20 000 points of the last plane lopsided along one axis: 29 of 30 at one end of the domain, the centroid lies
        # there and D is almost 2^24, so that 3 n D^2 = 1.6e19 >= 2^63
        k, a = 20_000, seed % 3
        xyz[:k] = rng.integers(-100, 101, (k, 3))
        xyz[:k, a] = np.where(np.arange(k) % 30 == 0, LIM, -LIM)
        plane[:k] = n_planes
    xyz, plane = layout(rng, xyz, plane, kind)
    return dict(xyz=xyz, plane_idx=plane, n_planes=n_planes, kind=kind)


def reach(c, fit):
    """the statuses and reduce regimes of DESIGN.md's table that the case reaches (pass A: every labelled point)"""
    plane, m = c["plane_idx"], c["n_planes"]
    out = {f"status{s}" for s in np.unique(fit.status)}
    n = len(plane)
    s = np.where((plane >= 1) & (plane <= m), plane - 1, -1).astype(np.int64)
    pad = np.full(-(-n // WAVE) * WAVE, -1, np.int64)
    pad[:n] = s
    w = pad.reshape(-1, WAVE)
    lab = w >= 0
    first = np.where(lab.any(1), w[np.arange(len(w)), lab.argmax(1)], -1)
    one = lab.any(1) & ((w == first[:, None]) | ~lab).all(1)
    if (one & (first < FIT_CAP)).any():
        out.add("wave_lds")
    if (one & (first >= FIT_CAP)).any():
        out.add("wave_global")
    many = w[~one & lab.any(1)]
    if ((many >= 0) & (many < FIT_CAP)).any():
        out.add("lane_lds")
    if (many >= FIT_CAP).any():
        out.add("lane_global")
    if n > TILE:
        out.add("workgroups>1")
    return out


REGIMES = {"status0", "status1", "status2", "wave_lds", "wave_global", "lane_lds", "lane_global", "workgroups>1"}
