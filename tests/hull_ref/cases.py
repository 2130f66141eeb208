"""Cases for the oriented boxes (include/bs_api.h, "oriented boxes"): label images of the stage's own, and those of
tests/outline_ref/cases.py and tests/facet_ref/cases.py by import.  A case is (label image, n_labels)."""
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
