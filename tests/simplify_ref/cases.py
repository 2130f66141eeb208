"""Cases for the simplified outlines (include/bs_api.h, "simplified outlines"): label images of the stage's own, the fuzz
cases and generators of tests/outline_ref/cases.py and tests/facet_ref/cases.py by import, the tolerances, and `regimes`:
which rows of the threshold table ("Simplified outlines") a case reaches, worked out from the references."""
from __future__ import annotations

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


oc = _load("outline_cases", os.path.join(HERE, "..", "outline_ref", "cases.py"))
sref = _load("simplify_ref", os.path.join(HERE, "simplify_ref.py"))
brute, fc, case = sref.brute, oc.fc, oc.case

TOLERANCES = ((0, 1), (1, 4), (1, 1), (2, 1), (25, 4), (10 ** 6, 1))
BIG_DEN = (1 << 31) - 1
LINE_SIZES = [s for n in (1, 2, 63, 64, 65) for s in ((1, n), (n, 1))]  # (width, height)
N_RANDOM = 60
REGIMES = ("closed_arc", "one_junction_node", "saddle", "junction_not_vertex", "tie_by_corner", "forced_split",
           "product_2_64", "rounds_8", "arc_without_interior", "no_pixel")


def _top(label, seed=0):
    """a top image that differs from pixel to pixel and corner to corner: a wrong pixel or corner shows"""
    rng = np.random.default_rng(4000 + seed)
    return rng.integers(-500, 500, np.shape(label) + (4,)).astype(np.int32)


def _c(label, seed=0):
    label = np.asarray(label, np.int32)
    return case(label, _top(label, seed), False)


def noisy_diagonal(n=40, seed=3):
    """two labels on either side of a diagonal that wobbles by a pixel"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:n, 0:n]
    return _c(np.where(xs + rng.integers(-1, 2, n)[:, None] > ys, 0, 1), seed)


def spiral(n=41):
    """one label in a one-pixel spiral: a single long arc whose splits go many rounds deep"""
    lab = np.full((n, n), -1, np.int32)
    x = y = 0
    dx, dy = 1, 0
    lab[0, 0] = 0
    while True:
        nx, ny = x + dx, y + dy
        ax, ay = nx + dx, ny + dy  # (the pixel after the next must be free, or the arm would touch the last lap)
        if not (0 <= nx < n and 0 <= ny < n) or lab[ny, nx] == 0 or (0 <= ax < n and 0 <= ay < n and lab[ay, ax] == 0):
            dx, dy = -dy, dx
            nx, ny = x + dx, y + dy
            ax, ay = nx + dx, ny + dy
            if not (0 <= nx < n and 0 <= ny < n) or lab[ny, nx] == 0 or (0 <= ax < n and 0 <= ay < n and lab[ay, ax] == 0):
                break
        x, y = nx, ny
        lab[y, x] = 0
    return _c(lab, 7)


def thin_l(n=400):
    """a one-pixel-thick L of n x n in front of a second label: the L's inner border is an open arc from (1, 0) to
    (n, n - 1) whose corner has |c| = (n - 1)^2: c^2 * den would pass 2^64 with den = 2^31 - 1, but the corner is the
    arc's first split, which is forced and not compared with the tolerance (thin_u puts such a product under it)"""
    lab = np.ones((n, n), np.int32)
    lab[:, 0] = 0
    lab[-1, :] = 0
    return case(lab, np.full((n, n, 4), 100, np.int32), True)


def thin_u(n=400):
    """the L with a third arm: the U's inner border is an open arc from (1, 0) to (n - 1, 0) with two corners of equal
    |c|; the first split is forced and takes the corner of the lower index, the other corner then stands against the
    tolerance with |c| = (n - 2)(n - 1), so c^2 * den passes 2^64 where the tolerance decides"""
    lab = np.ones((n, n), np.int32)
    lab[:, 0] = lab[:, -1] = 0
    lab[-1, :] = 0
    return case(lab, np.full((n, n, 4), 100, np.int32), True)


def own_shapes():
    """name -> case"""
    out = {"one_pixel": _c([[0]]), "rectangle": _c(np.zeros((5, 9)))}
    plus = np.full((9, 9), -1)
    plus[3:6, :] = 0
    plus[:, 3:6] = 0
    out["plus"] = _c(plus)
    side = np.zeros((6, 8))
    side[:, 4:] = 1
    out["side_by_side"] = _c(side)
    out["junction_in_run"] = _c([[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 2, 2], [1, 1, 2, 2]])
    out["saddle"] = _c([[0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0]])
    out["saddle_outside"] = _c([[0, 0, -1, -1], [0, 0, -1, -1], [-1, -1, 0, 0], [-1, -1, 0, 0]])
    out["saddle_joined"] = _c([[0, 0, 0], [0, -1, 0], [-1, 0, 0]])
    # a block and a pixel that touch in one corner: each ring passes that saddle once, its only junction node (the right
    # label of a ring can only change at a junction and has to change back, so a lone junction is always a saddle)
    out["one_junction"] = _c([[0, 0, -1], [0, 0, -1], [-1, -1, 0]])
    island = np.zeros((9, 9))
    island[3:6, 2:7] = 1
    out["island"] = _c(island)
    hole = np.zeros((7, 8))
    hole[2:5, 3:6] = -1
    out["hole"] = _c(hole)
    nest = np.zeros((9, 9))
    nest[2:7, 2:7] = -1
    nest[4, 4] = 1
    out["label_in_hole"] = _c(nest)
    out["noisy_diagonal"] = noisy_diagonal()
    out["spiral"] = spiral()
    out["nothing"] = _c(np.full((4, 6), -1))
    for w, h in LINE_SIZES:
        c = oc.line_case(w, h)
        out[f"line_{w}x{h}"] = dict(c, top=_top(c["label"], w + h))
    return out


def named_cases():
    yield from own_shapes().items()
    for seed in range(fc.N_FUZZ):
        yield f"fuzz_{seed}", oc.from_facet(fc.fuzz_case(seed))
    for seed in range(N_RANDOM):
        yield f"random_{seed}", oc.random_case(seed)


def big_cases():
    """(name, case, tolerances): cases with tolerances of their own"""
    yield "thin_l_400", thin_l(), ((BIG_DEN, BIG_DEN), (BIG_DEN // 4, BIG_DEN), (0, 1))
    yield "thin_u_400", thin_u(), ((BIG_DEN, BIG_DEN), (BIG_DEN // 4, BIG_DEN), (0, 1))


def all_runs():
    """(name, case, (num, den)) of everything the suites run"""
    for name, c in named_cases():
        for tol in TOLERANCES:
            yield name, c, tol
    for name, c, tols in big_cases():
        for tol in tols:
            yield name, c, tol


def run_ref(c, tol, trace=None):
    return sref.simplify(c["label"], c["top"], c["n_labels"], tol[0], tol[1], trace=trace)


def regimes(c, tol):
    """the rows of REGIMES this run reaches"""
    t = {}
    plain, s = run_ref(c, tol, t)
    if plain.n_half == 0:
        return {"no_pixel"}
    out = set()
    for key, name in (("closed_arcs", "closed_arc"), ("one_junction_rings", "one_junction_node"), ("saddles", "saddle"),
                      ("junction_not_vertex", "junction_not_vertex"), ("ties", "tie_by_corner"),
                      ("forced_only", "forced_split"), ("empty_arcs", "arc_without_interior")):
        if t[key] > 0:
            out.add(name)
    if t["max_product"] >= 1 << 64:
        out.add("product_2_64")
    if s.rounds >= 8:
        out.add("rounds_8")
    return out
