"""Cases for the model raster (include/bs_api.h, "model raster"): the runs of tests/triangulate_ref/cases.py by import, the
stage's own shapes, each with the tolerances it runs at, and `regimes`: which rows of the threshold table ("Model
raster") a run reaches, worked out from the restatement's result and trace."""
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
mref = _load("modelraster_ref", os.path.join(HERE, "modelraster_ref.py"))
boxwise = _load("modelraster_boxwise", os.path.join(HERE, "boxwise.py"))
brute, tref, tbrute, uref, sc = mref.brute, tc.tref, tc.brute, tc.uref, tc.sc

REGIMES = ("tie_owned", "tie_not_owned", "multi", "spill", "uncovered", "moved", "empty_span", "span_over_chunk", "failed_label",
           "labels_at_cap", "labels_above_cap", "no_pixel")
STRIPS = (mref.FIG_CAP - 1, mref.FIG_CAP, mref.FIG_CAP + 1, 5000)


def bay():
    """a block with a bay four pixels wide and an island of label 1 in the bay: at a coarse tolerance label 0's polygon
    closes the bay over the island, and no label fails"""
    lab = np.full((14, 14), -1, np.int32)
    lab[1:13, 1:13] = 0
    lab[1:9, 5:9] = -1
    lab[4, 7] = 1
    return sc._c(lab, 5)


def staircase(n=12):
    """two labels on either side of a one-pixel staircase diagonal: at (1, 1) the chord passes through every centre it
    crosses, so the tie rule decides each of those pixels"""
    ys, xs = np.mgrid[0:n, 0:n]
    return sc._c(np.where(xs >= ys, 0, 1), 6)


def wide():
    """one label of 3000 x 40: two triangles whose spans are longer than any workgroup chunk"""
    return sc._c(np.zeros((40, 3000), np.int32), 7)


def band(n=500):
    """two two-pixel-wide diagonal bands: at (2, 1) the straight one (label 0) is two slivers, one of them with 400 rows of a
    pixel or two, and the one that wobbles by a pixel (label 1) some hundred slivers with spans of 0 to 3"""
    ys, xs = np.mgrid[0:n, 0:n]
    lab = np.full((n, n), -1, np.int32)
    lab[(xs == ys + 100) | (xs == ys + 101)] = 0
    wob = np.random.default_rng(8).integers(0, 2, n)[:, None]
    lab[(xs >= ys - 100 + wob) & (xs <= ys - 99 + wob)] = 1
    return sc._c(lab, 8)


def strip(n):
    """n one-pixel labels in a row"""
    return sc._c(np.arange(n, dtype=np.int32).reshape(1, n), 14)


def own_shapes():
    """name -> (case, tolerances)"""
    t0 = ((0, 1),)
    shapes = {"bay": (bay(), ((0, 1), (100, 1), (10 ** 6, 1))), "staircase": (staircase(), ((0, 1), (1, 1))), "wide": (wide(), t0),
              "band": (band(), ((2, 1),)), "no_label_pixel": (dict(sc._c(np.full((3, 4), -1, np.int32), 15), n_labels=2), t0)}
    shapes.update({f"strip_{n}": (strip(n), t0) for n in STRIPS})
    return shapes


def all_runs():
    """(name, case, (num, den)) of everything the suites run"""
    yield from tc.all_runs()
    for name, (c, tols) in own_shapes().items():
        for tol in tols:
            yield name, c, tol


def regimes(tri, result, trace):
    """the regimes a run reaches: from the triangles' statuses, the restatement's result and its trace"""
    out = {k for k in ("tie_owned", "tie_not_owned") if trace.get(k, 0) > 0}
    for k, v in (("multi", result.n_multi), ("spill", result.n_spill), ("uncovered", result.n_uncovered), ("moved", result.n_moved),
                 ("empty_span", result.n_empty_spans)):
        if v > 0:
            out.add(k)
    if result.max_span > mref.CHUNK:
        out.add("span_over_chunk")
    failed = np.flatnonzero((np.asarray(tri.label_status) == tbrute.NO_BRIDGE) | (np.asarray(tri.label_status) == tbrute.STALLED))
    if len(failed) and result.pixels[failed].sum() > 0 and result.model_pixels[failed].sum() == 0:
        out.add("failed_label")
    nl = result.n_labels
    if nl == mref.FIG_CAP and result.model_pixels[nl - 1] > 0:
        out.add("labels_at_cap")
    if nl > mref.FIG_CAP and result.model_pixels[mref.FIG_CAP:].sum() > 0:
        out.add("labels_above_cap")
    if result.total_pixels == 0:
        out.add("no_pixel")
    return out
