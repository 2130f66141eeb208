"""Cases for the clean outlines (include/bs_api.h, "clean outlines"): the named cases and tolerances of
tests/simplify_ref/cases.py by import, shapes of the stage's own, and `regimes`: which rows of the threshold table
("Clean outlines") a run reaches, worked out from the references."""
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


sc = _load("simplify_cases", os.path.join(HERE, "..", "simplify_ref", "cases.py"))
uref = _load("uncross_ref", os.path.join(HERE, "uncross_ref.py"))
brute = uref.brute

TOLERANCES, BIG_DEN = sc.TOLERANCES, sc.BIG_DEN
CELL_LOG2 = (1, 3, 30)  # one corner pair per cell, many cells, one cell (the default, 4, runs in every other test)
REGIMES = ("cross", "touch", "overlap_at_shared_end", "marked_without_interior", "rounds_3", "no_conflict", "twin_pair",
           "span_100_cells")
# The runs of the named cases that conflict: the brute force over all of them finds exactly these.  The random images and
# the shapes of this stage's own ...
CONFLICTING = (("random_20", (25, 4)), ("random_56", (25, 4)), ("random_20", (10 ** 6, 1)), ("random_25", (10 ** 6, 1)),
               ("random_30", (10 ** 6, 1)), ("random_46", (10 ** 6, 1)), ("random_52", (10 ** 6, 1)), ("finger", (10 ** 6, 1)),
               ("finger_mirrored", (10 ** 6, 1)))
# ... and three of the 16 facet fuzz cases: fuzz_1 crosses, fuzz_2 and fuzz_10 touch, already at (2, 1).  (Images of
# thousands of segments: the suites run them at the smaller cell sizes, not with every segment in one cell.)
CONFLICTING_FUZZ = (("fuzz_1", (25, 4)), ("fuzz_1", (10 ** 6, 1)), ("fuzz_2", (2, 1)), ("fuzz_2", (25, 4)), ("fuzz_2", (10 ** 6, 1)),
                    ("fuzz_10", (2, 1)), ("fuzz_10", (25, 4)), ("fuzz_10", (10 ** 6, 1)))


def finger():
    """a comb of label 1 round a notch of label 0 with a finger of label 2 in it: the chords of the notch's arcs cut through
    the finger, and un-dropping one node per round takes three rounds to clear it"""
    lab = np.zeros((20, 30), np.int32)
    lab[2:18, 2:28] = 1
    lab[2:12, 10:20] = 0
    lab[2:14, 14:16] = 2
    return sc._c(lab, 5)


def own_shapes():
    """name -> case; the mirror image meets the same conflicts with other corner indices, so other ties"""
    f = finger()
    lab = np.ascontiguousarray(f["label"][:, ::-1])
    return {"finger": f, "finger_mirrored": sc._c(lab, 6)}


def named_cases():
    yield from sc.named_cases()
    yield from own_shapes().items()


def regimes(c, tol, cell_log2=0):
    t, u = {}, {}
    _, b = brute.clean(c["label"], c["top"], c["n_labels"], *tol, trace=t) if c["label"].size <= 900 else (None, None)
    _, _, r = uref.clean(c["label"], c["top"], c["n_labels"], *tol, cell_log2=cell_log2, trace=u)
    out = set()
    if b is not None:
        out |= {k for k in ("cross", "touch", "overlap_at_shared_end", "marked_without_interior") if t[k] > 0}
        if t["twin_pairs"] > 0:
            out.add("twin_pair")
    if r.repair_rounds >= 3:
        out.add("rounds_3")
    if r.n_marked_first == 0:
        out.add("no_conflict")
    if u.get("max_span", 0) >= 100:
        out.add("span_100_cells")
    return out
