"""Cases for the polygon solids (include/bs_api.h, "polygon solids"): the runs of tests/triangulate_ref/cases.py by import,
each with two building tables (every label in building 0; label % 3) and two base_z (below all tops; 0, in the middle of the
random tops), the stage's own shapes with hand-set tops, and `regimes`: which rows of the threshold table ("Polygon
solids") a run reaches, worked out from the restatement's trace."""
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


tc = _load("triangulate_cases", os.path.join(HERE, "..", "triangulate_ref", "cases.py"))
pref = _load("polysolid_ref", os.path.join(HERE, "polysolid_ref.py"))
brute, tref, tbrute, uref, sc = pref.brute, tc.tref, tc.brute, tc.uref, tc.sc

BASES = (-1000, 0)  # below every random top (-500 .. 499); in their middle
TABLES = ("one", "mod3")
BIN = 25
REGIMES = ("wall_3", "wall_4", "wall_6", "wall_8", "crossing", "between_up", "between_down", "twin_wall", "suppressed_twin",
           "base_wall", "other_building", "outside", "flush", "below_base", "column_of_5", "open_building", "empty_label",
           "empty_mesh", "buildings_at_cap", "buildings_above_cap")


def table(kind, n_labels):
    """(label_building, n_buildings)"""
    if kind == "one":
        return np.zeros(n_labels, np.int32), 1
    if kind == "mod3":
        return (np.arange(n_labels) % 3).astype(np.int32), 3
    if kind == "each":
        return np.arange(n_labels, dtype=np.int32), n_labels
    raise KeyError(kind)


def _shape(label, default, tops, n_labels=None):
    """a case with hand-set tops: every corner of a pixel of label l is default[l], then tops[(x, y, k)] = z overrides corner
    k (0: (x, y), 1: (x + 1, y), 2: (x, y + 1), 3: (x + 1, y + 1)) of pixel (x, y)"""
    label = np.asarray(label, np.int32)
    top = np.zeros(label.shape + (4,), np.int32)
    for (y, x), l in np.ndenumerate(label):
        top[y, x, :] = default[l] if l >= 0 else 0
    for (x, y, k), z in tops.items():
        top[y, x, k] = z
    c = sc.case(label, top, False)
    return dict(c, n_labels=c["n_labels"] if n_labels is None else n_labels)


def pair(a_s, a_e, b_s, b_e):
    """labels 0 | 1 side by side; label 0's segment s = (1, 0) -> e = (1, 1) has a_s, a_e on its own side, b_s, b_e on label
    1's"""
    return _shape([[0, 1]], {0: 300, 1: 200}, {(0, 0, 1): a_s, (0, 0, 3): a_e, (1, 0, 0): b_s, (1, 0, 2): b_e})


def six(mid):
    """2 x 3 pixels, six labels; the segment of label 2 against label 3 runs between two corners where four labels meet; mid:
    the heights of (label 0, 1 at the upper corner, label 4, 5 at the lower corner)"""
    lab = [[0, 1], [2, 3], [4, 5]]
    return _shape(lab, {l: 400 + 10 * l for l in range(6)},
                  {(0, 1, 1): 100, (0, 1, 3): 110, (1, 1, 0): 10, (1, 1, 2): 20,  # label 2: a_s, a_e; label 3: b_s, b_e
                   (0, 0, 3): mid[0], (1, 0, 2): mid[1], (0, 2, 1): mid[2], (1, 2, 0): mid[3]})


def four(z):
    """2 x 2 pixels, four labels that meet at the corner (1, 1) at the heights z"""
    return _shape([[0, 1], [2, 3]], {l: 300 + 10 * l for l in range(4)},
                  {(0, 0, 3): z[0], (1, 0, 2): z[1], (0, 1, 1): z[2], (1, 1, 0): z[3]})


def courtyard():
    lab = np.zeros((3, 3), np.int32)
    lab[1, 1] = -1
    return _shape(lab, {0: 250}, {(1, 0, 2): 240, (1, 0, 3): 260})


def strip(n):
    """n one-pixel labels in a row"""
    return sc._c(np.arange(n, dtype=np.int32).reshape(1, n), 14)


def own_shapes():
    """name -> (case, tolerances, ((table kind, base_z), ...))"""
    t0 = ((0, 1),)
    low = (("one", -1000),)
    return {
        "wall_3": (pair(50, 70, 50, 20), t0, low), "wall_4": (pair(50, 70, 20, 30), t0, low),
        "wall_flush": (pair(50, 70, 50, 70), t0, low), "wall_crossing": (pair(50, 20, 20, 50), t0, low + (("one", 30),)),
        "wall_between": (pair(50, 60, -50, -40), t0, (("one", 0),)), "wall_between_reversed": (pair(-50, -40, 50, 60), t0, (("one", 0),)),
        "wall_8": (six((70, 40, 80, 50)), t0, low + (("one", 60),)),
        "wall_other_building": (pair(50, 70, 20, 30), t0, (("each", -1000), ("each", 60))),
        "wall_below_base": (pair(50, 70, 20, 30), t0, (("one", 1000), ("each", 1000))),
        "courtyard": (courtyard(), t0, low),
        "corner_of_four": (four((10, 20, 30, 40)), t0, low + (("each", -1000), ("one", 25), ("mod3", 25))),
        "label_without_ring": (_shape([[0, 2]], {0: 100, 2: 150}, {}, n_labels=4), t0, low + (("mod3", 0),)),
        "no_label_pixel": (dict(sc._c(np.full((3, 4), -1, np.int32), 15), n_labels=2), t0, (("one", 0), ("mod3", 0))),
        "strip_1023": (strip(1023), t0, (("each", -1000),)), "strip_1024": (strip(1024), t0, (("each", -1000),)),
        "strip_1025": (strip(1025), t0, (("each", -1000),)), "strip_5000": (strip(5000), t0, (("each", -1000),)),
    }


def all_runs():
    """(name, case, (num, den), table kind, base_z) of everything the suites run"""
    for name, c, tol in tc.all_runs():
        for kind in TABLES:
            for base in BASES:
                yield name, c, tol, kind, base
    for name, (c, tols, variants) in own_shapes().items():
        for tol in tols:
            for kind, base in variants:
                yield name, c, tol, kind, base


def regimes(tri, lb, nb, trace, result):
    """the regimes a run reaches: from the triangles' statuses, the table, the restatement's trace and its result"""
    out = set()
    sizes = set(trace.get("wall_sizes", ()))
    out |= {f"wall_{k}" for k in (3, 4, 6, 8) if k in sizes}
    for k, r in (("between_up", "between_up"), ("between_down", "between_down"), ("n_twin_walls", "twin_wall"),
                 ("n_suppressed", "suppressed_twin"), ("n_base_walls", "base_wall"), ("other_building", "other_building"),
                 ("outside", "outside"), ("n_flush", "flush"), ("below_base", "below_base"), ("columns_of_5", "column_of_5")):
        if trace.get(k, 0) > 0:
            out.add(r)
    if result.n_crossing_walls > 0:
        out.add("crossing")
    if result.n_open_buildings > 0 and result.n_faces > 0:
        out.add("open_building")
    if (np.asarray(tri.label_status) == tbrute.EMPTY).any() and result.n_faces > 0:
        out.add("empty_label")
    if result.n_vertices == 0 and result.n_faces == 0:
        out.add("empty_mesh")
    if nb == pref.FIG_CAP and result.wall_faces[nb - 1] > 0:
        out.add("buildings_at_cap")
    if nb > pref.FIG_CAP and result.wall_faces[pref.FIG_CAP:].sum() > 0:
        out.add("buildings_above_cap")
    return out
