"""Cases for the sweeps of the clean outlines (include/bs_api.h, "clean outlines", paragraph "Sweeps"): the runs of
tests/triangulate_ref/cases.py and tests/modelraster_ref/cases.py by import, the stage's own shapes, each with the tolerances
it runs at, and `regimes`: which rows of the threshold table ("Sweeps") a run reaches, worked out from the
restatement's figures."""
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


mc = _load("modelraster_cases", os.path.join(HERE, "..", "modelraster_ref", "cases.py"))
wref = _load("sweep_ref", os.path.join(HERE, "sweep_ref.py"))
tc, sc, uref, tref, tbrute, boxwise = mc.tc, mc.sc, mc.uref, mc.tref, mc.tbrute, mc.boxwise
brute = wref.brute

BIG = (10 ** 6, 1)
REGIMES = ("sweeping", "sweeping_only", "sweeping_and_conflicting", "two_sweep_rounds", "rays_along_y",
           "rays_along_x", "hit_rejected", "path_over_wave_cap", "winding_2", "lens_without_hit")
# runs that break the outcome promise (a label without a bridge, a stall or n_multi > 0 after the repair in mode 2), each
# with the reason: (name, tolerance) -> reason.  The test asserts that the exceptions are exactly these.
OUTCOME_EXCEPTIONS = {}


def transposed(c):
    """the case mirrored at the diagonal (top's four corner heights keep their places: the stage reads them as they are)"""
    return dict(c, label=np.ascontiguousarray(c["label"].T), top=np.ascontiguousarray(np.transpose(c["top"], (1, 0, 2))))


def deep_bay():
    """a block with a deep bay and an island of label 1 low in the bay: at a coarse tolerance the outer ring's chord closes
    the bay over the island, and the first repair leaves a chord that still does"""
    lab = np.full((30, 30), -1)
    lab[1:29, 1:29] = 0
    lab[1:24, 8:22] = -1
    lab[21, 19] = 1
    return sc._c(lab, 21)


def s_curve():
    """two labels whose border makes an S, an island in either bulge: the border's two twins both sweep, and the round
    after has conflicts and sweeps at once"""
    lab = np.zeros((40, 24))
    lab[:, 12:] = 1
    lab[6:16, 12:18] = 0
    lab[24:34, 6:12] = 1
    lab[10, 15] = 2
    lab[28, 8] = 3
    return sc._c(lab, 22)


def zigzag_bay(teeth=40):
    """a bay whose floor is a comb of `teeth` teeth: the outer ring's path around the bay has more than 64 runs; an island
    in the bay"""
    wd = 2 * teeth + 5
    lab = np.full((12, wd), -1)
    lab[1:11, 1:wd - 1] = 0
    lab[1:8, 2:wd - 2] = -1
    lab[6:8, 3:wd - 2:2] = 0  # the teeth
    lab[3, teeth] = 1
    return sc._c(lab, 24)


def two_lobes():
    """the border of two labels from the left edge to the right: a bulge up, a bulge down, then a spike that the forced
    split keeps: the chord from the left end to the spike crosses its own path between the bulges, and the island in either
    bulge is swept with the opposite sign"""
    lab = np.zeros((21, 24))
    lab[10:, :] = 1
    lab[6:10, 4:10] = 1     # label 1 bulges up
    lab[10:14, 10:16] = 0   # label 0 bulges down
    lab[5:10, 20] = 1       # the spike
    lab[8, 6] = 2
    lab[11, 13] = 3
    return sc._c(lab, 25)


def spiral_arc(size=31, margin=3, pitch=4, turns=11):
    """a one-pixel slit of label 1 that enters label 0 from the left edge, closes one lap around the middle and spirals on
    inwards to an island of label 2 on its end: chords of the slit's sides wind around kept corners twice"""
    lab = np.zeros((size, size))
    box = [margin, margin, size - 1 - margin, size - 1 - margin]  # left, top, right, bottom
    x, y = 0, size // 2
    pts = [(x, y), (margin, y)]
    x = margin
    for t in range(turns):  # up, right, down, left, ... each leg to the box's side, which then moves in
        side = (1, 2, 3, 0)[t % 4]
        if side % 2:
            y = box[side]
        else:
            x = box[side]
        pts.append((x, y))
        if t >= 2:
            box[(3, 0, 1, 2)[t % 4]] += pitch if t % 4 in (1, 2) else -pitch
    for (x0, y0), (x1, y1) in zip(pts, pts[1:]):
        lab[min(y0, y1):max(y0, y1) + 1, min(x0, x1):max(x0, x1) + 1] = 1
    (x0, y0), (x1, y1) = pts[-2], pts[-1]
    lab[y1 + np.sign(y1 - y0), x1 + np.sign(x1 - x0)] = 2  # the island on the slit's end
    return sc._c(lab, 26)


def wobbly_stripes(n=700, height=3, seed=31):
    """stripes of labels 0 and 1, `height` pixels tall, that all follow one random walk from column to column: every border
    is one arc from the left edge to the right with some n dropped nodes, and strays from its chord by more than the
    stripes' height -- more items and candidate corners than one sweep of a grid-stride pass, and lenses that hold the kept
    nodes of the borders beside them"""
    rng = np.random.default_rng(seed)
    walk = np.cumsum(rng.integers(-1, 2, n))
    ys, xs = np.mgrid[0:n, 0:n]
    return sc._c(((ys + (walk - walk.min())[xs]) // height) % 2, seed)


def noise(n=600, share=0.8, seed=12):
    """noise that is mostly label 0: more nodes and more segments than one sweep of a grid-stride pass"""
    rng = np.random.default_rng(seed)
    lab = rng.integers(-1, 3, (n, n))
    return dict(sc._c(np.where(rng.random((n, n)) < share, 0, lab), seed), n_labels=3)


# the runs of tests/triangulate_ref/cases.py of at most 900 pixels in which a segment sweeps: (name, tolerance)
SWEEPING_RUNS = (("random_0", BIG), ("random_20", (25, 4)), ("random_20", BIG), ("random_25", BIG), ("random_30", BIG),
                 ("random_46", BIG), ("random_56", (25, 4)), ("finger", BIG), ("finger_mirrored", BIG))


def own_shapes():
    """name -> (case, tolerances)"""
    db = deep_bay()
    return {"deep_bay": (db, ((100, 1), BIG)), "deep_bay_t": (transposed(db), ((100, 1), BIG)),
            "s_curve": (s_curve(), ((25, 1), (100, 1), BIG)),
            "zigzag_bay": (zigzag_bay(), (BIG,)), "two_lobes": (two_lobes(), ((100, 1), BIG)),
            "spiral_arc": (spiral_arc(), (BIG,))}


def all_runs():
    """(name, case, (num, den)) of everything the suites run"""
    yield from mc.all_runs()
    for name, (c, tols) in own_shapes().items():
        for tol in tols:
            yield name, c, tol


def regimes(res, trace):
    """the regimes a run of the restatement in mode 2 reaches: from its figures and the figures of its detections"""
    out = set()
    det = trace.get("detections", [])
    if res.n_sweeping_first > 0:
        out.add("sweeping")
    if res.n_sweeping_only_first > 0:
        out.add("sweeping_only")
    if any(d["n_sweeping"] > d["n_only"] for d in det):
        out.add("sweeping_and_conflicting")
    if res.sweep_rounds >= 2:
        out.add("two_sweep_rounds")
    if res.n_items_first > res.n_items_swapped_first:
        out.add("rays_along_y")
    if res.n_items_swapped_first > 0:
        out.add("rays_along_x")
    if res.n_rejected_first > 0:
        out.add("hit_rejected")
    if res.n_exact_wave_first > 0:
        out.add("path_over_wave_cap")
    if res.max_abs_winding >= 2:
        out.add("winding_2")
    if res.n_lens_segments_first > 0 and res.n_exact_first == 0:
        out.add("lens_without_hit")
    return out
