"""Cases for the facet outlines (include/bs_api.h, "facet outlines"): the cases of tests/facet_ref/cases.py, each run
through the facet reference for its facet image and top, label images of the stage's own, and `regimes`: which rows of
the threshold table ("Facet outlines") a case reaches, worked out from its label image and the reference."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


fc = _load("facet_cases", os.path.join(HERE, "..", "facet_ref", "cases.py"))
orf = _load("outline_ref", os.path.join(HERE, "outline_ref.py"))
brute = orf.brute

N_RANDOM = 60  # random label images whose labels are not connected components
LINE_SIZES = [(1, 1)] + [s for n in (2, 63, 64, 65, 257) for s in ((1, n), (n, 1))]  # (width, height)
REGIMES = ("ring_of_4", "every_pixel_a_ring", "corner_twice", "hole", "hole_touches_outer", "label_in_hole",
           "start_not_a_vertex", "three_rings", "n_half_power_of_two", "n_half_power_of_two_plus_2", "border_all_sides",
           "no_pixel", "long_ring")


def case(label, top=None, connected=True, facets=None):
    """a case of this stage: the label image, top (or None), whether every label is one 4-connected component, and the
    facet reference's result where the image is its facet image"""
    label = np.ascontiguousarray(label, np.int32)
    return dict(label=label, top=None if top is None else np.ascontiguousarray(top, np.int32),
                n_labels=max(int(label.max()) + 1, 0), connected=connected, facets=facets)


def from_facet(c):
    """a facet case as an outline case: the facet image of the facet reference and the case's top"""
    r = fc.run_ref(c)
    return dict(case(r.facet, c["top"], True, r), n_labels=int(r.n_facets))


def _flat_top(label, z=100):
    return np.full(label.shape + (4,), z, np.int32)


def wide_hole():
    """6 x 5, one label, a hole two pixels wide: the hole's lowest half-edge lies in the middle of a straight run"""
    lab = np.zeros((5, 6), np.int32)
    lab[2, 2:4] = -1
    return case(lab, _flat_top(lab))


def own_shapes():
    """name -> case: the label images of this stage's own"""
    out = {"wide_hole": wide_hole()}
    lab = np.array([[0, -1, -1], [0, 0, -1], [-1, 0, 0], [-1, -1, 0]])  # (a staircase: no corner twice, for contrast)
    out["staircase"] = case(lab, _flat_top(lab))
    lab = np.array([[0, 0, 0], [0, -1, 0], [-1, 0, 0]])  # two diagonal pixels joined elsewhere: the ring visits (1, 2) twice
    out["corner_twice"] = case(lab, _flat_top(lab))
    # ring_with_hole with the hole moved into the corner: the hole pixel (1, 1) and the notch (0, 0) meet at the lattice
    # corner (1, 1).  The left-turn rule keeps the two label pixels there apart, so the hole opens into the outside: ONE
    # ring that visits the corner twice, and no hole ring.
    ring = np.zeros((5, 5), np.int32)
    ring[0, 0] = -1
    ring[1, 1] = -1
    out["hole_touches_outer"] = case(ring, _flat_top(ring))
    ring = np.zeros((5, 5), np.int32)
    ring[2, 2] = 1  # a label inside a hole of another
    out["label_in_hole"] = case(ring, _flat_top(ring))
    plate = np.zeros((5, 9), np.int32)
    plate[2, 2] = plate[2, 6] = -1
    out["two_holes"] = case(plate, _flat_top(plate))
    for n in (31, 32):  # 2 * n + 2 half-edges in one ring: 64 and 66
        out[f"strip_{n}"] = case(np.zeros((1, n), np.int32), _flat_top(np.zeros((1, n))))
    out["full_image"] = case(np.zeros((7, 9), np.int32), _flat_top(np.zeros((7, 9))))
    out["nothing"] = case(np.full((4, 6), -1, np.int32), _flat_top(np.zeros((4, 6))))
    return out


def serpentine(n=257):
    """one label that winds through every second row of n x n, joined at alternating ends: a single ring"""
    lab = np.full((n, n), -1, np.int32)
    lab[0::2, :] = 0
    lab[1::4, -1] = 0
    lab[3::4, 0] = 0
    return case(lab, _flat_top(lab, 250))


def random_case(seed):
    """a random label image of at most 12 x 12 whose labels are scattered: not connected components"""
    rng = np.random.default_rng(21000 + seed)
    h, w = (int(v) for v in rng.integers(1, 13, 2))
    nl = int(rng.integers(1, 5))
    lab = rng.integers(-1, nl, (h, w)).astype(np.int32)
    if seed % 5 == 0:
        lab = np.where(rng.random((h, w)) < 0.8, 0, lab).astype(np.int32)  # mostly one label: holes and diagonal contact
    top = rng.integers(-500, 500, (h, w, 4)).astype(np.int32)
    return dict(case(lab, top, False), n_labels=nl)


def line_case(w, h):
    """1 x N and N x 1 images: runs of two labels and gaps along the line"""
    rng = np.random.default_rng(w * 1000 + h)
    lab = np.repeat(rng.integers(-1, 2, w * h // 3 + 1), 3)[:w * h].reshape(h, w).astype(np.int32)
    return dict(case(lab, _flat_top(lab), False), n_labels=2)


def named_cases():
    """(name, case): the named shapes of the facet cases and this stage's own"""
    for name, c in fc.named_shapes().items():
        yield name, from_facet(c)
    for name, c in own_shapes().items():
        yield name, c


def all_cases():
    """(name, case) of everything the regime test looks at"""
    yield from named_cases()
    for seed in range(fc.N_SOLID_FUZZ):
        yield f"solid_fuzz_{seed}", from_facet(fc.solid_fuzz_case(seed))
    for seed in range(fc.N_FUZZ):
        yield f"fuzz_{seed}", from_facet(fc.fuzz_case(seed))
    yield "serpentine_257", serpentine()


def run_ref(c):
    return orf.outlines(c["label"], c["top"], c["n_labels"])


def regimes(c, o=None):
    """the rows of REGIMES this case reaches"""
    label = np.asarray(c["label"], np.int64)
    h, w = label.shape
    o = run_ref(c) if o is None else o
    if o.n_half == 0:
        return {"no_pixel"}
    out = set()
    if (o.ring_length == 4).any():
        out.add("ring_of_4")
    if o.n_rings == (label >= 0).sum() and o.n_rings > 1:
        out.add("every_pixel_a_ring")
    hole = o.ring_area2 < 0
    if hole.any():
        out.add("hole")
    if (np.diff(o.label_ring_offset) >= 3).any():
        out.add("three_rings")
    for r in range(o.n_rings):
        pts = o.xy[o.ring_offset[r]:o.ring_offset[r + 1]]
        if len(np.unique(pts, axis=0)) < len(pts):
            out.add("corner_twice")
            # a 4-connected piece of the complement that does not reach the image border (a hole by pixels) and meets
            # another piece at such a corner: it has no ring of its own
            lr = int(o.ring_label[r])
            comp = ndimage.label(np.pad(label != lr, 1, constant_values=True))[0]
            a, b, cc, d = comp[:-1, :-1], comp[:-1, 1:], comp[1:, :-1], comp[1:, 1:]
            for u, v in ((a, d), (b, cc)):
                if ((u > 0) & (v > 0) & (u != v) & ((u != comp[0, 0]) | (v != comp[0, 0]))).any():
                    out.add("hole_touches_outer")
        # a ring's start is a vertex iff its first listed vertex is the start corner of h0
        p, k = divmod(int(o.ring_start[r]), 4)
        if tuple(pts[0]) != (p % w + orf.SX[k], p // w + orf.SY[k]):
            out.add("start_not_a_vertex")
    # a label whose outer ring lies inside a hole's box and is no larger than the hole
    for r in np.nonzero(hole)[0]:
        x0, y0, x1, y1 = o.ring_bbox[r]
        inside = label[y0:y1, x0:x1]
        if ((inside >= 0) & (inside != o.ring_label[r])).any() and c["connected"]:
            other = np.unique(inside[(inside >= 0) & (inside != o.ring_label[r])])
            for l2 in other:  # the other label lies wholly inside the hole's box and touches only the hole's label or itself
                b = o.ring_bbox[o.label_ring_offset[l2]]
                if b[0] >= x0 and b[1] >= y0 and b[2] <= x1 and b[3] <= y1 and -o.ring_area2[r] >= o.ring_area2[o.label_ring_offset[l2]]:
                    out.add("label_in_hole")
    if o.n_rings == 1 and o.n_half & (o.n_half - 1) == 0:
        out.add("n_half_power_of_two")
    if o.n_rings == 1 and (o.n_half - 2) & (o.n_half - 3) == 0:
        out.add("n_half_power_of_two_plus_2")
    bb = o.ring_bbox
    if (bb[:, 0] == 0).any() and (bb[:, 1] == 0).any() and (bb[:, 2] == w).any() and (bb[:, 3] == h).any():
        out.add("border_all_sides")
    if o.ring_length.max() >= 1 << 16:
        out.add("long_ring")
    assert out <= set(REGIMES), out - set(REGIMES)
    return out
