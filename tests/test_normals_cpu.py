"""The normals' floating-point tail on the CPU: tests/normal_ref against the C oracle and against 60-digit arithmetic.

1. trace.py (a third transcription of SURVEY.md A.2 / A.3, in Python floats) equals oracle.fast_eigen3x3 and
   oracle.normal_from_list bit for bit on every neighbourhood of the committed case list and on hand-made matrices.
2. The committed list reaches every leaf in cases.REQUIRED at least three times; the table is printed (pytest -s).
3. The accuracy of the reference algorithm against exact.py stays inside an envelope per family.
4. Norm and orientation of every result.
"""
import collections
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "fit_ref")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from normal_ref import cases, exact, trace  # noqa: E402
import fit_ref as fr  # noqa: E402

# Measured with the oracle against mpmath on the committed list (cases.envelope): the worst
#   factor = sin(angle) * (l1 - l0) / (l2 * 2^-52)  against the eigenvector of the f64 covariance, both placements
#   sin    = sin(angle)                               against the eigenvector of the exact covariance, 'near' (< 4.2 m)
# per family.  Asserted: 4 x the measured value, rounded up to a power of two -- the margin covers the one ulp a change
# of bs_detmath.h may still move inside its 2-ulp pin.  lattice: the covariance is exactly diagonal, the answer an axis.
MEASURED = {
    # family:      (factor,   sin)
    "blob":        (1.630,    5.40e-12),
    "patch":       (1.403,    1.66e-12),
    "collinear":   (23118.0,  3.67e-09),
    "lattice":     (0.0,      0.0),
    "isotropic":   (1.473,    3.78e-10),
    "needle":      (1125.3,   2.49e-08),
    "pancake":     (0.02687,  2.28e-12),
    "ident":       (0.7249,   5.50e-08),
    "wall":        (0.5093,   2.00e-12),
    "sheet":       (0.01341,  1.38e-12),
    "tri":         (1.462,    1.70e-11),
}
ASSERTED = {
    "blob":        (8.0,      2.0 ** -35),
    "patch":       (8.0,      2.0 ** -37),
    "collinear":   (131072.0, 2.0 ** -26),
    "lattice":     (0.0,      0.0),
    "isotropic":   (8.0,      2.0 ** -29),
    "needle":      (8192.0,   2.0 ** -23),
    "pancake":     (0.125,    2.0 ** -36),
    "ident":       (4.0,      2.0 ** -22),
    "wall":        (4.0,      2.0 ** -36),
    "sheet":       (0.0625,   2.0 ** -37),
    "tri":         (8.0,      2.0 ** -33),
}
MAX_DROPPED = 0.02  # of a non-degenerate family's placed clusters the gap filter may leave out

# matrices no integer neighbourhood was found for: the leaves the case list does not reach, where a matrix reaches them
EXTRA_MATRICES = [
    [0.0] * 6,
    [-1.0, -2.0, -3.0, -1.5, -2.5, -0.5],        # every entry negative: negmax
    [-2.0, -1.0, -1.0, -2.0, -1.0, -2.0],
    [2.0, 1.0, 0.0, 2.0, 0.0, 1.0],              # eigenvalues 1, 1, 3
    [2.0, 1.0, 1.0, 2.0, 1.0, 2.0],              # eigenvalues 1, 1, 4
    [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],              # rank one
    [4.0, 2.0, 0.0, 1.0, 0.0, 0.0],              # rank one in a plane
    [1.0, 0.0, 0.0, 2.0, 0.0, 3.0], [3.0, 0.0, 0.0, 1.0, 0.0, 2.0], [3.0, 0.0, 0.0, 2.0, 0.0, 1.0],
    [1.0, 0.0, 0.0, 1.0, 0.0, 1.0], [2.0, 0.0, 0.0, 1.0, 0.0, 1.0],
    [1.0, 1e-170, 0.0, 2.0, 0.0, 3.0],           # off-diagonal whose square underflows: the diagonal branch
    [1.0, 1e-160, 0.0, 2.0, 0.0, 3.0],           # ... and one that just does not
    [1e-300, 1e-301, 0.0, 2e-300, 0.0, 3e-300], [1e300, 1e299, 2e299, 2e300, 1e298, 3e300],
]


def _pow2_ceil(x):
    return 0.0 if x == 0 else 2.0 ** math.ceil(math.log2(x))


def _placed_all():
    clusters, leaves = cases.case_list()
    for i, c in enumerate(clusters):
        for where in ("near", "domain"):
            yield c, where, cases.placed(c, i, cases.PITCH, where), leaves[i][where]


def _same_bits(a, b):
    return np.array_equal(trace.bits(a), trace.bits(b))


def test_trace_equals_the_oracle_bit_for_bit(oracle):
    n = 0
    for c, where, pts, leaves in _placed_all():
        c6 = trace.cov_of(pts.tolist())
        v, lv = trace.fast_eigen3x3(c6)
        assert _same_bits(v, oracle.fast_eigen3x3(c6)), (c["name"], where, lv)
        idx = np.arange(len(pts), dtype=np.int32)
        tail, lv2 = trace.normal_of_points(pts.tolist())
        assert lv2 == lv == leaves
        assert _same_bits(tail, oracle.normal_from_list(pts.astype(np.int32), idx)), (c["name"], where, lv)
        n += 1
    assert n == 2 * len(cases.case_list()[0])
    # fewer than three points: the identity, through the diagonal branch
    two = np.array([[5, 6, 7], [9, 9, 9]], np.int32)
    assert trace.normal_of_points(two.tolist()) == ([0.0, 0.0, 1.0], ("diag.z",))
    assert _same_bits([0.0, 0.0, 1.0], oracle.normal_from_list(two, np.arange(2, dtype=np.int32)))


def test_trace_equals_the_oracle_on_hand_made_matrices(oracle):
    """Leaves outside the case list's reach, NaN patterns included.  Printed: which leaves these matrices take."""
    rng = np.random.default_rng(cases.SEED)
    mats = list(EXTRA_MATRICES)
    for _ in range(300):  # symmetric matrices that are no covariance: indefinite, negative, badly scaled
        mats.append((rng.normal(size=6) * 10.0 ** rng.integers(-8, 9)).tolist())
    seen = collections.Counter()
    for c6 in mats:
        v, lv = trace.fast_eigen3x3(c6)
        assert _same_bits(v, oracle.fast_eigen3x3(c6)), (c6, lv)
        seen.update(set(lv))
    print("\nhand-made matrices:", {l: seen[l] for l in trace.LEAVES if seen[l]})
    assert seen["zero"] and seen["negmax"] and seen["diag.x"] and seen["diag.y"] and seen["diag.z"]


def _fit_leaves(oracle):
    """the leaves of the covariance the plane fit forms (deviations from the integer centroid) with every cluster of
    the 'near' cloud labelled as one plane"""
    xyz, cid, sizes = cases.committed_cloud("near")
    rec = []

    def eigen(c6):
        rec.append(trace.fast_eigen3x3(c6)[1])
        return oracle.fast_eigen3x3(c6)

    f = fr.plane_fit(xyz, (cid + 1).astype(np.int32), len(sizes), eigen=eigen)
    assert (f.status == 0).all() and len(rec) == len(sizes)
    return rec


def test_leaf_coverage(oracle):
    clusters, leaves = cases.case_list()
    count = {w: collections.Counter() for w in ("near", "domain", "fit")}
    paths = collections.Counter()
    for lv in leaves:
        for w, t in lv.items():
            count[w].update(set(t))
            paths[t] += 1
    for t in _fit_leaves(oracle):
        count["fit"].update(set(t))
        paths[t] += 1
    print("\n%-8s %6s %6s %6s   (clusters: %d, leaf paths: %d)" % ("leaf", "near", "domain", "fit", len(clusters), len(paths)))
    for l in trace.LEAVES:
        print("%-8s %6d %6d %6d%s" % (l, count["near"][l], count["domain"][l], count["fit"][l],
                                      "" if l in cases.REQUIRED else "   (not required)"))
    for t, c in sorted(paths.items(), key=lambda kv: -kv[1]):
        print("%5d  %s" % (c, " ".join(t)))
    assert set(cases.REQUIRED) | set(cases.UNREACHED) == set(trace.LEAVES)
    for l in cases.REQUIRED:
        assert count["near"][l] + count["domain"][l] >= cases.MIN_PER_LEAF, l
    # a leaf outside REQUIRED that the list does reach belongs into REQUIRED
    for l in cases.UNREACHED:
        assert count["near"][l] + count["domain"][l] + count["fit"][l] == 0, "%s is reached: add it to REQUIRED" % l


def test_accuracy_envelope(oracle):
    """Measured (oracle against mpmath, committed list) and asserted = 4 x measured, rounded up to a power of two:

    family      factor measured / asserted     sin measured / asserted (exact covariance, 'near')
    blob          1.630   / 8                   5.40e-12 / 2^-35
    patch         1.403   / 8                   1.66e-12 / 2^-37
    collinear     23118   / 131072              3.67e-09 / 2^-26
    lattice       0       / 0                   0        / 0
    isotropic     1.473   / 8                   3.78e-10 / 2^-29
    needle        1125.3  / 8192                2.49e-08 / 2^-23
    pancake       0.02687 / 0.125               2.28e-12 / 2^-36
    ident         0.7249  / 4                   5.50e-08 / 2^-22
    wall          0.5093  / 4                   2.00e-12 / 2^-36
    sheet         0.01341 / 0.0625              1.38e-12 / 2^-37
    tri           1.462   / 8                   1.70e-11 / 2^-33
    """
    for f in cases.FAMILIES:
        assert ASSERTED[f] == tuple(_pow2_ceil(4 * m) for m in MEASURED[f]), f

    def from_points(pts):
        a = np.array(pts, np.int32)
        return oracle.normal_from_list(a, np.arange(len(a), dtype=np.int32))

    env = cases.envelope(oracle.fast_eigen3x3, from_points)
    print()
    for f in cases.FAMILIES:
        e = env[f]
        print("%-10s factor %-12.5g sin %-12.4g placed %3d dropped %3d" % (f, e["factor"], e["sin"], e["n"], e["dropped"]))
    for f in cases.FAMILIES:
        e = env[f]
        assert e["factor"] <= ASSERTED[f][0], (f, e)
        assert e["sin"] <= ASSERTED[f][1], (f, e)
        if f in cases.NON_DEGENERATE:
            assert e["dropped"] <= MAX_DROPPED * e["n"], (f, e)


def test_norm_and_orientation(oracle):
    for c, where, pts, leaves in _placed_all():
        n = oracle.normal_from_list(pts.astype(np.int32), np.arange(len(pts), dtype=np.int32))
        if np.isnan(n).any():
            continue
        assert abs(math.sqrt(float(n @ n)) - 1) < 1e-12, (c["name"], where, n)
        assert n[2] >= 0, (c["name"], where, n)
        if leaves == ("zero",):
            assert _same_bits(n, [0.0, 0.0, 1.0]), (c["name"], where, n)


def test_clouds_keep_their_premises():
    """cloud() asserts the separation with integers; here: the sizes, and what the special clouds are built for"""
    clusters, _ = cases.case_list()
    assert 200 <= len(clusters) <= cases.SLOTS and all(3 <= len(c["pts"]) <= 64 for c in clusters)
    for where in ("near", "domain"):
        xyz, cid, sizes = cases.committed_cloud(where)
        assert 5000 <= len(xyz) <= 20000 and np.array_equal(np.bincount(cid), sizes)
    assert np.abs(cases.committed_cloud("domain")[0]).max() == (1 << 23) - 2
    for max_nn in (3, 50, 64):
        xyz, cid, sizes, k = cases.boundary_cloud(max_nn)
        assert sorted(set(sizes.tolist())) == [max_nn - 1, max_nn, max_nn + 1] and sizes.min() >= k
    # corner cloud: with the grid at the bounding box and 7 500 mm cells, every point's third neighbour is two cells
    # away on every axis, in the far corner of the 5 x 5 x 5 block
    xyz, radius = cases.corner_cloud(7500)
    x = xyz.astype(np.int64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    third = np.argsort(d2, axis=1, kind="stable")[:, 2]
    assert (np.abs(x // 7500 - x[third] // 7500) == 2).all()
    assert (np.sort(d2, axis=1)[:, 2] < radius * radius).all() and (np.sort(d2, axis=1)[:, 3] > radius * radius).all()
