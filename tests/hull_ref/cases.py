"""Cases for the oriented boxes (include/bs_api.h, "oriented boxes"): label images of the stage's own, and those of
tests/outline_ref/cases.py and tests/facet_ref/cases.py by import.  A case is (label image, n_labels); the sparse cases at the
end of the file (a few single pixels in an image of thousands of pixels across) are pixel lists, see there."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if "hull_ref" not in sys.modules:
    _spec = importlib.util.spec_from_file_location("hull_ref", os.path.join(HERE, "hull_ref.py"))
    sys.modules["hull_ref"] = importlib.util.module_from_spec(_spec)
    _spec.loader.exec_module(sys.modules["hull_ref"])
ref = sys.modules["hull_ref"]

brute = ref.brute
oc = ref._load("outline_cases", os.path.join(HERE, "..", "outline_ref", "cases.py"))
fc = oc.fc

# radius -> (n_hull, best_edge): the lowest of the tied edges, edge i leaving vertex i of the list (tests/test_hulls_cpu.py
# relates them to the figures of the issue, which counts the same edges from the list's second vertex)
DISCS = {2: (8, 1), 5: (16, 1), 12: (24, 3), 60: (64, 8), 100: (72, 1)}
PARABOLAS = (10, 58, 59, 60, 61, 62, 63, 64, 65)  # j: j + 5 hull vertices (63, 64, 65: the lanes of the box pass wrap)
ROTATED = (((4, 3), 100, 50, 140), ((4, 3), 41, 17, 70), ((2, 1), 60, 30, 90), ((1, 1), 40, 20, 60), ((5, 2), 80, 33, 110),
           ((7, 3), 33, 20, 60))  # (direction, long side, short side, image size)
LINE_SIZES = oc.LINE_SIZES


def case(label, n_labels=None):
    label = np.ascontiguousarray(label, np.int32)
    return label, max(int(label.max()) + 1, 0) if n_labels is None else int(n_labels)


def disc(r):
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return case(np.where(x * x + y * y <= r * r, 0, -1))


def parabola(j):
    """single pixels at (i, i (i + 1) / 2), i = 0 .. j"""
    lab = np.full((j * (j + 1) // 2 + 1, j + 1), -1, np.int32)
    i = np.arange(j + 1)
    lab[i * (i + 1) // 2, i] = 0
    return case(lab)


def rotated(direction, long_side, short_side, n):
    """a rectangle along `direction`, centred at n / 2, rasterised by pixel centre"""
    d = np.array(direction, np.float64) / np.hypot(*direction)
    y, x = np.mgrid[0:n, 0:n]
    u, v = x + 0.5 - n / 2, y + 0.5 - n / 2
    return case(np.where((np.abs(u * d[0] + v * d[1]) <= long_side / 2) & (np.abs(-u * d[1] + v * d[0]) <= short_side / 2), 0, -1))


def bound():
    """16385 x 2: row 0 is label 0 (beyond the bound), the first 16383 pixels of row 1 are label 1 (just within)"""
    lab = np.full((2, 16385), -1, np.int32)
    lab[0, :] = 0
    lab[1, :16383] = 1
    return case(lab)


def small_shapes():
    """name -> case: the smallest shapes"""
    out = {"one_pixel": case(np.zeros((1, 1)))}
    for w, h in LINE_SIZES:
        out[f"full_line_{w}x{h}"] = case(np.zeros((h, w)))
        c = oc.line_case(w, h)
        out[f"runs_line_{w}x{h}"] = case(c["label"], c["n_labels"])
    out["full_rectangle"] = case(np.zeros((5, 9)))
    out["square"] = case(np.pad(np.zeros((6, 6), np.int32), 2, constant_values=-1))
    lab = np.full((7, 7), -1)
    lab[1:6, 1:3] = lab[4:6, 1:6] = 0
    out["L"] = case(lab)
    lab = np.full((9, 9), -1)
    lab[3:6, 1:8] = lab[1:8, 3:6] = 0
    out["plus"] = case(lab)
    y, x = np.mgrid[-7:8, -7:8]
    out["diamond"] = case(np.where(np.abs(x) + np.abs(y) <= 7, 0, -1))
    out["corner_touch"] = case(np.array([[0, -1], [-1, 0]]))
    lab = np.zeros((7, 8))
    lab[2:5, 2:6] = -1
    out["ring_shaped"] = case(np.pad(lab.astype(np.int32), 1, constant_values=-1))
    lab = np.full((40, 50), -1)
    lab[1:3, 2:5] = lab[30:38, 40:48] = lab[20, 3] = 0
    lab[10:14, 20:30] = 1
    out["three_far_pieces"] = case(lab)
    y, x = np.mgrid[0:8, 0:8]
    out["checkerboard"] = case((x + y) % 2)
    lab = np.full((6, 12), -1)
    lab[1:3, 1:4], lab[2:5, 6:11] = 1, 4
    out["unused_labels"] = case(lab, 7)
    out["nothing"] = case(np.full((4, 6), -1), 3)
    lab = np.full((9, 11), -1)
    lab[4, :] = lab[:, 5] = 0
    out["touches_all_borders"] = case(lab)
    return out


def moved(c, dx, dy):
    lab, nl = c
    return case(np.pad(lab, ((dy, 1), (dx, 2)), constant_values=-1), nl)


def named_cases():
    """(name, case) of everything but the large images"""
    yield from small_shapes().items()
    for r in DISCS:
        yield f"disc_{r}", disc(r)
    for j in PARABOLAS:
        yield f"parabola_{j}", parabola(j)
    for d, a, b, n in ROTATED:
        yield f"rotated_{d[0]}_{d[1]}_{a}x{b}", rotated(d, a, b, n)
    for name, c in oc.own_shapes().items():
        yield "outline_" + name, case(c["label"], c["n_labels"])


def fuzz_cases():
    """the random labels of the outline suite and the facet fuzz images"""
    for seed in range(oc.N_RANDOM):
        c = oc.random_case(seed)
        yield f"random_{seed}", case(c["label"], c["n_labels"])
    for seed in range(fc.N_FUZZ):
        c = oc.from_facet(fc.fuzz_case(seed))
        yield f"facet_fuzz_{seed}", case(c["label"], c["n_labels"])


def serpentine():
    c = oc.serpentine()
    return case(c["label"], c["n_labels"])


def blobs():
    """1025 x 1027: more than one grid sweep of the outline passes, more than 1 000 rings"""
    c = oc.from_facet(fc.blob_case(1025, 1027, seed=5, size=40, nb=700))
    return case(c["label"], c["n_labels"])


def run_ref(c):
    return ref.label_hulls(*c)


def run_brute(c):
    return brute.label_hulls(*c)


# ---- sparse cases: a few single pixels in a large image -------------------------------------------------------------------
# A sparse case is dict(width, height, pixels [[x, y, label]]).  The two references take the pixel list; only a test that
# asks the device builds the image.
def sparse(width, height, pixels):
    return dict(width=int(width), height=int(height), pixels=np.array(pixels, np.int64).reshape(-1, 3))


def n_labels_of(s):
    return int(s["pixels"][:, 2].max()) + 1


def dense(s):
    lab = np.full((s["height"], s["width"]), -1, np.int32)
    lab[s["pixels"][:, 1], s["pixels"][:, 0]] = s["pixels"][:, 2]
    return lab, n_labels_of(s)


def transposed(s):
    return sparse(s["height"], s["width"], s["pixels"][:, [1, 0, 2]])


def beside(s, pixels, first=False):
    """the case with a second label of the given pixels [(x, y)]: label 1, or label 0 with the others moved up"""
    p = s["pixels"].copy()
    p[:, 2] += bool(first)
    return sparse(s["width"], s["height"], np.concatenate([p, [(x, y, 0 if first else n_labels_of(s)) for x, y in pixels]]))


def sparse_brute(s):
    return brute.pixel_hulls(*s["pixels"].T, s["width"], s["height"], n_labels_of(s))


def sparse_ref(s):
    return ref.pixel_hulls(*s["pixels"].T, s["width"], s["height"], n_labels_of(s))


def octagon(f, side):
    """eight single pixels, two on every side of a side x side image, at the fractions f[0..7] of the side"""
    m = side - 1
    at = [int(round(v * m)) for v in f]
    return sparse(side, side, [(at[0], 0, 0), (at[1], 0, 0), (m, at[2], 0), (m, at[3], 0), (at[4], m, 0), (at[5], m, 0),
                               (0, at[6], 0), (0, at[7], 0)])


def diamond(c, n=0, d=0):
    """single pixels at the four tips of a diamond of half-diagonal c; n > 0: every tip is an arc of 2 n + 1 pixels
    (c + d t, t^2), t = -n .. n, turned about the centre to the other three (d > 2 n keeps the arcs inside the long edges)"""
    top = [(c + d * t, t * t) for t in range(-n, n + 1)]
    pix = []
    for _ in range(4):
        pix += top
        top = [(2 * c - y, x) for x, y in top]
    return sparse(2 * c + 1, 2 * c + 1, [(x, y, 0) for x, y in pix])


def from_dense(c):
    ys, xs = np.nonzero(c[0] >= 0)
    return sparse(c[0].shape[1], c[0].shape[0], np.stack([xs, ys, c[0][ys, xs]], axis=1))


SMALL_LABEL = ((0, 0), (1, 0), (0, 1))  # an L of three pixels, for the second label of an image
# Found by search over octagon() with random.Random(seed): tests/test_hulls_cpu.py asserts what each was searched for.
LADDER_SIDES = (1024, 1200, 1500, 2048, 4096)
LADDER_F = (0.511, 0.776, 0.108, 0.449, 0.247, 0.096, 0.702, 0.522)  # every pair of the best edge: < 2^64 at 1024, high words differ at 4096
HIGH_WORD_F = (0.409, 0.943, 0.082, 0.262, 0.577, 0.305, 0.857, 0.534)  # side 3000: edge 5 beats every edge by the low words, edge 3 is least
CLASS_C = ((903, 0), (1144, 0), (2047, 374), (2047, 778), (1232, 2047), (815, 2047), (0, 778), (0, 373))  # mirror images but for (2047, 374)
FULL_BOUND = ((0, 0), (16382, 16382), (5861, 14663), (493, 15536), (959, 3829), (2253, 15833), (4879, 9759))
STRIP = ((0, 0), (9100, 310), (16382, 2047), (7200, 1750), (3000, 900))
# Found by search over chains of segments whose lengths grow by a constant factor near 2 while they turn (QuickHull then takes
# one vertex per round): (width, height, pixels); the number is the count of rounds the restatement gives.
ROUND_CHAINS = {
    5: (29, 196, ((0, 0), (1, 0), (3, 1), (6, 3), (8, 195), (11, 8), (18, 20), (26, 46), (28, 97))),
    8: (436, 692, ((0, 691), (316, 362), (412, 0), (413, 0), (415, 1), (415, 174), (419, 4), (425, 12), (432, 32), (435, 78))),
    9: (929, 377, ((0, 376), (542, 320), (789, 209), (889, 118), (917, 0), (918, 0), (920, 1), (922, 60), (923, 4), (926, 11),
                   (928, 28))),
    13: (9746, 10916, ((0, 10915), (5861, 6501), (8355, 3663), (9331, 1980), (9653, 0), (9655, 1), (9659, 4), (9663, 1035),
                       (9666, 11), (9677, 26), (9694, 58), (9717, 125), (9741, 260), (9745, 525))),
}


def one_label(width, height, pixels):
    return sparse(width, height, [(x, y, 0) for x, y in pixels])


def strip():
    """16385 x 2050: label 0 beyond the bound (two pixels 16385 apart in the last row), label 1 within it with corners at
    (0, 0) and (16383, 2048) and oblique edges between"""
    return sparse(16385, 2050, [(0, 2049, 0), (16384, 2049, 0)] + [(x, y, 1) for x, y in STRIP])


def rounds_1_5_9():
    """labels of 1, 5 and 9 rounds in one image: the first two sit idle through the batches of the third"""
    pix = [(1100, 10, 0)] + [(1000 + x, y, 1) for x, y in ROUND_CHAINS[5][2]] + [(x, y, 2) for x, y in ROUND_CHAINS[9][2]]
    return sparse(1110, 377, pix)


def magnitude_cases():
    """name -> sparse case: the compared products around and above 2^64, the coordinates at the bound"""
    out = {f"ladder_{s}": octagon(LADDER_F, s) for s in LADDER_SIDES}
    out["high_word"] = octagon(HIGH_WORD_F, 3000)
    out["high_word_beside"] = beside(out["high_word"], [(1500 + x, 1400 + y) for x, y in SMALL_LABEL])
    out["class_c"] = one_label(2048, 2048, CLASS_C)
    out["tie_diamond"] = diamond(1500)
    out["tie_diamond_beside"] = beside(out["tie_diamond"], [(1500 + x, 1500 + y) for x, y in SMALL_LABEL], first=True)
    out["tie_diamond_lanes"] = diamond(1500, 11, 24)
    out["tie_diamond_same_lane"] = diamond(2040, 15, 32)
    out["bound_transposed"] = transposed(from_dense(bound()))
    out["shallow"] = one_label(16383, 4, [(16382, 0), (0, 1), (9000, 3)])  # (the next row's corner index is lower only by its row)
    out["shallow_transposed"] = transposed(out["shallow"])
    out["strip"] = strip()
    out["strip_transposed"] = transposed(strip())
    return out


def round_cases():
    out = {f"rounds_{r}": one_label(*c) for r, c in ROUND_CHAINS.items()}
    out["rounds_1_5_9"] = rounds_1_5_9()
    return out


def full_bound(side=16383):
    """one label whose box is side x side, in an image of the next power of two (16384 x 16384: 1 GiB of int32)"""
    size = 1 << (side - 1).bit_length()
    return one_label(size, size, [(x * (side - 1) // 16382, y * (side - 1) // 16382) for x, y in FULL_BOUND])


FUZZ_SIDES = (1150, 2048, 4096)
N_SPARSE_FUZZ = 20


def sparse_fuzz(seed):
    """1 to 3 labels of 3 to 40 single pixels; both sides within 3 of one of FUZZ_SIDES, or one of them within 3 of the bound"""
    rng = np.random.default_rng([seed, 0x68756c6c])
    w, h = (int(rng.choice(FUZZ_SIDES)) + int(rng.integers(-3, 4)) for _ in range(2))
    at_bound = int(rng.integers(0, 3))  # 0: neither side, 1: the width, 2: the height
    if at_bound == 1:
        w = brute.MAX_SIDE + int(rng.integers(-3, 4))
    elif at_bound == 2:
        h = brute.MAX_SIDE + int(rng.integers(-3, 4))
    pix = []
    for l in range(int(rng.integers(1, 4))):
        n = int(rng.integers(3, 41))
        pix += [(int(x), int(y), l) for x, y in zip(rng.integers(0, w, n), rng.integers(0, h, n))]
    taken = {}
    for x, y, l in pix:  # (a pixel has one label: the first that drew it)
        taken.setdefault((x, y), l)
    return sparse(w, h, [(x, y, l) for (x, y), l in taken.items()])
