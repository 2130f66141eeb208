"""Seeded neighbourhoods that reach every leaf of the eigen-solver, and the clouds that carry them through the kernels.

The device: a CLUSTER is 3 to 64 integer points inside a box of edge BOX (its diameter is below RADIUS).  Clusters sit
on a coarse lattice whose pitch keeps every two of them further apart than RADIUS plus the largest diameter, so the
hybrid neighbourhood (d^2 < r^2, at most max_nn points) of every point of a cluster of at most max_nn points is
exactly the cluster: all its points share one covariance and must carry the same normal, bit for bit, and which
neighbourhood reaches which leaf of the solver is known on the CPU (trace.py) before any kernel runs.

case_list() is the committed list: PER_FAMILY clusters of each family from one seed, then a seeded search that keeps
drawing clusters until every leaf in REQUIRED is taken by at least MIN_PER_LEAF of the list's placed clusters.  The
search only picks inputs -- it calls the traced restatement, never the code under test.  Slot i of the list has a fixed
place in both placements, so the leaves a cluster takes (they depend on where it lies: the cumulants cancel) are fixed.

cloud(clusters, pitch, where): 'near' starts the lattice at the origin; 'domain' hangs 3 x 3 x 3 sub-lattices on the
eight corners, the six face centres and the centre of |c| <= 2^23 - 2, so one grid spans the whole admissible domain.
"""
import functools
import itertools
import math

import numpy as np

from . import trace

RADIUS = 181.0            # the largest radius of the REL32 moment path
BOX = 100                 # local coordinates 0 .. BOX: diameter <= 100 sqrt(3) = 173.3 < 181
PITCH = 500               # gap between boxes >= 400 > RADIUS + 173.3
LIM = (1 << 23) - 2
SEED = 20261
PER_FAMILY = 30
SLOTS = 405               # 15 sites x 27 in 'domain', 9 x 9 x 5 in 'near'
MIN_PER_LEAF = 3
FAMILIES = ("blob", "patch", "collinear", "lattice", "isotropic", "needle", "pancake", "ident", "wall", "sheet", "tri")
NON_DEGENERATE = ("blob", "patch", "isotropic", "needle", "pancake", "wall", "sheet")

# Leaves every change of the solver must keep reaching.  Not required, because no neighbourhood was found that takes
# them: negmax, e0.zero, e1.tie01, e1.U0, e1.U1 and the returns h+.v2, h+.v1, h-.v1, h-.x.  For three of those there is an
# argument: angle = acos(h) / 3 lies in [0, pi/3], so beta0 = 2 cos(angle + 2 pi / 3) <= -1 <= beta1 <= 1 <= beta2
# = 2 cos(angle) and, for h < 0, beta0 < -sqrt(3) < 0 < beta1: with p > 0, q + p beta2 is never strictly below
# q + p beta0 (h+.v2), and for h < 0 q + p beta0 is always strictly the smallest (h-.v1 and h-.x need it not to be).
# The ties e0.tie and e1.tie are reached (collinear runs, equilateral triangles) and required; e1.tie01 was not found.
REQUIRED = ("zero", "diag.x", "diag.y", "diag.z", "clamp+", "clamp-", "h+", "h-", "e0.0", "e0.1", "e0.2", "e0.tie", "e1.Ux",
            "e1.Uy", "e1.tie", "e1.a", "e1.b", "e1.c", "e1.d", "h+.x", "h-.v0")
UNREACHED = ("negmax", "e0.zero", "e1.tie01", "e1.U0", "e1.U1", "h+.v2", "h+.v1", "h-.v1", "h-.x")

SITES = [s for s in itertools.product((-1, 0, 1), repeat=3) if sum(abs(a) for a in s) in (0, 1, 3)]
assert len(SITES) == 15 and SLOTS == len(SITES) * 27 == 9 * 9 * 5


def _fit(p):
    return np.clip(np.rint(p), 0, BOX).astype(np.int64)


def _rot(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def draw(family, rng):
    """one cluster of the family: int64 [m, 3] in 0 .. BOX, 3 <= m <= 64"""
    m = int(rng.integers(4, 65))
    if family == "blob":  # (with two opposite corners of the box: the outermost blobs of 'domain' touch +-LIM)
        return np.concatenate([rng.integers(0, BOX + 1, (m - 2, 3)), [[0, 0, 0], [BOX, BOX, BOX]]])
    if family == "patch":
        uv = rng.uniform(-45, 45, (m, 2))
        p = np.concatenate([uv, rng.uniform(-2, 2, (m, 1))], 1)
        return _fit(p @ _rot(rng).T / math.sqrt(2) * 1.2 + BOX / 2)
    if family == "collinear":
        while True:
            d = rng.integers(-4, 5, 3)
            if d.any():
                break
        tmax = int(min(BOX // abs(a) for a in d if a))
        m = int(rng.integers(3, min(24, tmax + 1) + 1))
        t = np.sort(rng.choice(tmax + 1, m, replace=False))
        p = np.where(d < 0, BOX, 0) + t[:, None] * d
        if rng.integers(3) == 0:  # one point one unit off the line
            p[rng.integers(m), rng.integers(3)] += 1
        return _fit(p)
    if family == "lattice":
        # full product grids with power-of-two counts: every cumulant is exact, the covariance exactly diagonal
        while True:
            cnt = rng.choice([1, 2, 4], 3)
            if 4 <= cnt.prod() <= 64:
                break
        sp = rng.choice([2, 6, 6, 10, 20], 3)
        ax = [np.arange(c) * s for c, s in zip(cnt, sp)]
        return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3) + rng.integers(0, 20, 3)
    if family == "isotropic":
        p = rng.uniform(-1, 1, (m, 3)) * rng.uniform(0.8, 1.0, 3) * 28
        return _fit(p @ _rot(rng).T + BOX / 2)
    if family in ("needle", "pancake"):
        perm = rng.permutation(3)
        p = np.empty((m, 3), np.int64)
        wide, thin = int(rng.integers(60, BOX + 1)), int(rng.integers(1, 4))
        ext = (wide, thin, thin) if family == "needle" else (wide, wide, thin)
        for a, e in zip(perm, ext):
            p[:, a] = rng.integers(0, e + 1, m) + rng.integers(0, BOX - e + 1)
        return p
    if family == "ident":
        m = int(rng.integers(3, 65)) if rng.integers(2) else int(rng.integers(56, 65))
        p = np.tile(rng.integers(1, BOX, 3), (m, 1))
        for _ in range(int(rng.integers(0, 3))):
            p[rng.integers(m), rng.integers(3)] += rng.choice([-1, 1])
        return p
    if family == "wall":
        phi, u = rng.uniform(0, math.pi), rng.uniform(-45, 45, m)
        p = np.stack([u * math.cos(phi), u * math.sin(phi), rng.uniform(-45, 45, m)], 1) + rng.uniform(-1, 1, (m, 3))
        return _fit(p + BOX / 2)
    if family == "sheet":
        return np.concatenate([rng.integers(0, BOX + 1, (m, 2)), rng.integers(40, 42, (m, 1))], 1)
    if family == "tri":
        if rng.integers(3) == 0:  # the cyclic shifts of one triple: an equilateral triangle, two equal largest eigenvalues
            a, b, c = rng.integers(0, BOX + 1, 3).tolist()
            return np.array([[a, b, c], [b, c, a], [c, a, b]], np.int64)
        return rng.integers(0, BOX + 1, (3, 3))
    raise ValueError(family)


def slot_origin(i, pitch, where, box=BOX):
    """where the box of slot i starts (Python integers)"""
    if where == "near":
        return [(i % 9) * pitch, (i // 9 % 9) * pitch, (i // 81) * pitch]
    assert where == "domain"
    site, sub = SITES[i % 15], i // 15
    u = [sub % 3 * pitch, sub // 3 % 3 * pitch, sub // 9 * pitch]
    ext = 2 * pitch + box  # (sub-lattice 0 is the outermost one)
    return [u[a] - ext // 2 if site[a] == 0 else (LIM - box - u[a] if site[a] > 0 else -LIM + u[a]) for a in range(3)]


def placed(cluster, i, pitch=PITCH, where="near", scale=1):
    return np.asarray(cluster["pts"], np.int64) * scale + np.array(slot_origin(i, pitch, where, BOX * scale), np.int64)


def leaves_of(cluster, i):
    """the leaves the cluster takes at slot i, in either placement of the committed clouds -> {where: tuple}"""
    return {w: trace.normal_of_points(placed(cluster, i, PITCH, w).tolist())[1] for w in ("near", "domain")}


def draw_list(rng, per_family=PER_FAMILY):
    """per_family clusters of every family, family by family"""
    return [{"family": f, "pts": draw(f, rng), "name": "%s.%d" % (f, j)} for f in FAMILIES for j in range(per_family)]


@functools.lru_cache(maxsize=None)
def case_list():
    """-> (clusters, leaves): clusters[i] = {'family', 'pts' (local int64 [m, 3]), 'name'}, leaves[i] = {where: tuple}"""
    rng = np.random.default_rng(SEED)
    clusters = draw_list(rng) + REGRESSIONS
    leaves = [leaves_of(c, i) for i, c in enumerate(clusters)]
    count = {l: 0 for l in trace.LEAVES}
    for lv in leaves:
        for t in lv.values():
            for l in set(t):
                count[l] += 1
    tries = 0
    while any(count[l] < MIN_PER_LEAF for l in REQUIRED):
        assert len(clusters) < SLOTS and tries < 20000, ("the search ran out", {l: count[l] for l in REQUIRED})
        tries += 1
        c = {"family": FAMILIES[tries % len(FAMILIES)], "name": "search.%d" % tries}
        c["pts"] = draw(c["family"], rng)
        lv = leaves_of(c, len(clusters))
        hit = {l for t in lv.values() for l in t}
        if any(count[l] < MIN_PER_LEAF for l in hit if l in REQUIRED):
            clusters.append(c)
            leaves.append(lv)
            for t in lv.values():
                for l in set(t):
                    count[l] += 1
    return clusters, leaves


# neighbourhoods that once made a kernel and the oracle differ, by name (none so far)
REGRESSIONS = []


def check_premises(blocks, radius, min_points=3, k=3):
    """blocks: the placed clusters (int64 arrays).  Integer arithmetic only."""
    r2 = radius * radius
    diam2 = 0
    for p in blocks:
        assert len(p) >= min_points
        d = p[:, None, :] - p[None, :, :]
        d2 = int((d * d).sum(-1).max())
        assert d2 < r2, "a cluster is wider than the radius"
        diam2 = max(diam2, d2)
    lo, hi = np.array([p.min(0) for p in blocks]), np.array([p.max(0) for p in blocks])
    gap = np.maximum(0, np.maximum(lo[:, None, :] - hi[None, :, :], lo[None, :, :] - hi[:, None, :]))
    g2 = (gap * gap).sum(-1)
    g2[np.arange(len(blocks)), np.arange(len(blocks))] = np.iinfo(np.int64).max
    need = math.isqrt(diam2) + 1 + math.ceil(radius)   # > radius + largest diameter
    assert int(g2.min()) > need * need, "two clusters are too close"
    assert sum(len(p) for p in blocks) >= k


def assemble(blocks, seed):
    """shuffle the points of the placed clusters -> xyz int32 [n, 3], cluster id [n], sizes [clusters]"""
    xyz = np.concatenate(blocks)
    assert np.abs(xyz).max() <= LIM
    cid = np.repeat(np.arange(len(blocks)), [len(p) for p in blocks])
    perm = np.random.default_rng(seed).permutation(len(xyz))
    return np.ascontiguousarray(xyz[perm], dtype=np.int32), cid[perm], np.array([len(p) for p in blocks])


def cloud(clusters, pitch=PITCH, where="near", scale=1, radius=None, k=3):
    """-> (xyz, cid, sizes) with the premises asserted for radius (default RADIUS * scale)"""
    blocks = [placed(c, i, pitch, where, scale) for i, c in enumerate(clusters)]
    check_premises(blocks, RADIUS * scale if radius is None else radius, k=k)
    xyz, cid, sizes = assemble(blocks, SEED + len(blocks))
    if where == "domain":
        assert (xyz.max(0) == LIM).all() and (xyz.min(0) == -LIM).all()
    return xyz, cid, sizes


@functools.lru_cache(maxsize=None)
def committed_cloud(where, pitch=PITCH, scale=1):
    return cloud(case_list()[0], pitch, where, scale)


@functools.lru_cache(maxsize=None)
def boundary_cloud(max_nn):
    """Clusters of max_nn - 1, max_nn and max_nn + 1 points (six of each, blobs and clumps with equal distances at the
    cut).  The points of an oversize cluster do not share a neighbourhood: each keeps its nearest max_nn by
    (d^2, index).  -> (xyz, cid, sizes, k): k = 2 where a cluster has two points, else 3."""
    rng = np.random.default_rng(SEED + max_nn)
    blocks = []
    for j in range(18):
        m = max_nn - 1 + j % 3
        if j % 2:   # a clump on a small lattice: many equal distances, and duplicates
            p = rng.integers(0, 4, (m, 3)) * 7 + rng.integers(0, BOX - 21, 3)
        else:
            p = rng.integers(0, BOX + 1, (m, 3))
        blocks.append(p.astype(np.int64) + np.array(slot_origin(j, PITCH, "near"), np.int64))
    k = 2 if max_nn == 3 else 3
    check_premises(blocks, RADIUS, min_points=max_nn - 1, k=k)
    return assemble(blocks, SEED + max_nn) + (k,)


def corner_cloud(cell=7500):
    """A sparse cloud for the cell edge at which the fast kernels are still allowed (5 * cell <= 37 500): triples A, B, C
    with A in the last corner of cell (2, 2, 2) of a block and B, C in the first corner of cell (0, 0, 0), and the mirror
    image -- the third neighbour of every point lies in the far corner of its 5 x 5 x 5 block, 3 * (3 * cell - 1)^2 away.
    -> (xyz, radius): the radius holds the whole triple."""
    far = 3 * cell - 1
    blocks = []
    for ix, iy, iz in itertools.product(range(3), repeat=3):
        base = np.array([ix, iy, iz], np.int64) * 16 * cell
        t = np.array([[far, far, far], [0, 0, 0], [5, 3, 0]], np.int64)
        if (ix + iy + iz) % 2:
            t = far - t
        blocks.append(t + base)
    xyz = np.concatenate(blocks)
    assert (xyz.min(0) == 0).all()
    perm = np.random.default_rng(SEED).permutation(len(xyz))
    radius = float(math.isqrt(3 * far * far) + 2)
    assert radius * radius < 2 ** 32 and radius < 16 * cell - far
    return np.ascontiguousarray(xyz[perm], dtype=np.int32), radius


def envelope(eigen, normal_from_points):
    """The accuracy of eigen (c6 -> vector) and normal_from_points (integer points -> normal) on the committed list
    against exact.py -> {family: {'factor': worst sin * (l1 - l0) / (l2 * 2^-52) against the eigenvector of the f64
    covariance, both placements; 'sin': worst plain sin against the eigenvector of the exact covariance, 'near' only;
    'n': placed clusters; 'dropped': those the gap filter left out}}"""
    from . import exact
    clusters, _ = case_list()
    out = {}
    for i, c in enumerate(clusters):
        e = out.setdefault(c["family"], {"factor": 0.0, "sin": 0.0, "n": 0, "dropped": 0})
        for where in ("near", "domain"):
            pts = placed(c, i, PITCH, where).tolist()
            c6 = trace.cov_of(pts)
            v, lam = exact.of_matrix(c6)
            e["n"] += 1
            if not exact.gap_ok(lam):
                e["dropped"] += 1
                continue
            n = [float(t) for t in eigen(c6)]
            assert not any(math.isnan(t) for t in n), c["name"]
            e["factor"] = max(e["factor"], float(exact.factor(n, v, lam)))
            if where == "near":
                v2, lam2 = exact.of_points(pts)
                if exact.gap_ok(lam2):
                    e["sin"] = max(e["sin"], float(exact.sin_angle(normal_from_points(pts), v2)))
    return out
