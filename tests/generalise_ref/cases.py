"""Cases for the roof generalisation (include/bs_api.h, "roof generalisation"): the named shapes, seeded fuzz, and
`regimes`: which rows of the threshold table ("Roof generalisation") a case reaches, worked out from the
restatement alone.  A case is the input of tests/solid_ref/cases.py plus `params`."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generalise_ref as gr  # noqa: E402

fr, sr, brute = gr.fr, gr.sr, gr.brute


def _solid_cases():
    """tests/solid_ref/cases.py under a name of its own (this directory has a cases.py too)"""
    if "solid_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("solid_cases", os.path.join(HERE, "..", "solid_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["solid_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["solid_cases"]


sc = _solid_cases()
KEYS = sc.KEYS
FIG_CAP, PLANE_CAP = 1024, 1024  # BS_GEN_FIG_CAP, BS_GEN_PLANE_CAP of include/bs_api.h
N_SMALL, N_FUZZ = 80, 28
# seeds of fuzz_case found by search (tests/tools/fuzz_generalise.py --search); the tests assert what they are for
SEED_WAITS, SEED_THREE_ROUNDS, SEED_FLAT_LATER = 5, 26, 8
SIZES = sorted({s for a in (1, 63, 64, 65, 129) for s in ((a, 17), (17, a))} | {(65, 17), (17, 65)})
REGIMES = ("stays_without_neighbour", "stays_unroofed_neighbour_only", "moves_small", "moves_flat", "unroofed_moves",
           "unroofed_value_kept", "length_tie", "chain_of_two", "waits_then_moves", "three_rounds", "flat_only_later",
           "two_buildings_touch", "diagonal_contact", "round_cap", "no_pixels", "building_lds", "building_global", "plane_lds",
           "plane_global", "tile_seam_x", "tile_seam_y")


def params(min_pixels=0, merge_flat=False, step_tol=200, bend_tol=0, max_rounds=64):
    return dict(min_pixels=int(min_pixels), merge_flat=bool(merge_flat), step_tol=int(step_tol), bend_tol=int(bend_tol),
                max_rounds=int(max_rounds))


def with_params(c, **kw):
    out = dict(c)
    out["params"] = params(**{**c.get("params", {}), **kw})
    return out


def run_ref(c):
    return gr.generalise(*[c[k] for k in KEYS], **c["params"])


def run_brute(c):
    return brute.generalise(*[c[k] for k in KEYS], **c["params"])


def _shape(bmap, roof, zs=(100, 200), normal=None, center=None, nb=None, bin=10, keep_roof=False, **kw):
    """a named shape: flat planes at the heights zs (or the tables given), clamps that never decide, base_z 0, flat 50"""
    bmap = np.asarray(bmap)
    n = len(zs) if normal is None else len(normal)
    if normal is None:
        normal, center = np.tile([0.0, 0.0, 1.0], (n, 1)), np.stack([np.zeros(n), np.zeros(n), np.asarray(zs)], 1)
    nb = int(bmap.max()) + 1 if nb is None else nb
    c = sc.make(bmap, roof, nb, normal, center, np.full(n, -10 ** 6), np.full(n, 10 ** 6), bin, 0, np.full(nb, 50))
    if keep_roof:  # (make() writes -1 outside every building; inside, 0 and -1 both stay as given)
        c["roof"] = np.where(c["bmap"] < 0, -1, np.asarray(roof, np.int32)).astype(np.int32)
    c["params"] = params(**kw)
    return c


def strip(n, **kw):
    """1 x n pixels of one building, planes 1 and 2 alternating: with min_pixels = 2 every facet chains west to pixel 0"""
    return _shape(np.zeros((1, n)), 1 + np.arange(n)[None, :] % 2, **{"min_pixels": 2, **kw})


def checkerboard(w, h, **kw):
    yy, xx = np.mgrid[0:h, 0:w]
    return _shape(np.zeros((h, w)), 1 + (yy + xx) % 2, **{"min_pixels": 2, **kw})


def caps_case(nb, npl):
    """nb buildings of two pixels side by side in one row, planes drawn from 1 .. npl so that the highest ones are used:
    the second pixel of every building joins the first"""
    bmap = np.repeat(np.arange(nb), 2)[None, :]
    k = np.arange(2 * nb)
    roof = (npl - (k % min(npl, 7)))[None, :]
    return _shape(bmap, roof, zs=100 + np.arange(npl), nb=nb, min_pixels=2)


def named_shapes():
    out = {}
    out["one_pixel"] = _shape([[0]], [[1]], min_pixels=4)
    out["one_facet"] = _shape(np.zeros((3, 3)), np.ones((3, 3)), min_pixels=100, merge_flat=True)
    out["two_pixels_two_planes"] = _shape([[0, 0]], [[1, 2]], min_pixels=2)
    isl = np.ones((5, 5), np.int64)
    isl[2, 2] = 2
    out["island"] = _shape(np.zeros((5, 5)), isl, min_pixels=2)
    for name, v in (("unroofed_island_0", 0), ("unroofed_island_m1", -1)):
        isl = np.ones((5, 5), np.int64)
        isl[2, 2] = v
        isl[0, 0:2] = -1 - v  # two unroofed pixels of the other value: not small, their value must survive
        out[name] = _shape(np.zeros((5, 5)), isl, keep_roof=True, min_pixels=2)
    out["small_beside_unroofed_only"] = _shape([[0, 0, 0, 0]], [[0, 0, 0, 1]], min_pixels=2)
    # a 1-pixel facet that touches four arms by one edge each; the corners lie outside the building
    plus = np.full((5, 5), -1, np.int64)
    plus[2, :] = 0
    plus[:, 2] = 0
    arms = np.zeros((5, 5), np.int64)
    arms[0:2, 2], arms[2, 0:2], arms[2, 3], arms[3:5, 2], arms[2, 2] = 1, 2, 3, 4, 5
    plus_eq = plus.copy()
    plus_eq[2, 4] = -1
    out["length_tie_equal_pixels"] = _shape(plus_eq, arms, zs=(100, 200, 300, 400, 500), min_pixels=2)
    arms2 = arms.copy()
    arms2[2, 3:5] = 3
    plus3 = plus.copy()
    plus3[0, 2] = -1  # the north arm has one pixel, east two (a third pixel hangs below it), south and west two
    plus3[3, 4] = 0
    arms2[3, 4] = 3
    out["length_tie_most_pixels"] = _shape(plus3, arms2, zs=(100, 200, 300, 400, 500), min_pixels=2)
    out["two_small_facets"] = _shape([[0, 0, 0]], [[1, 1, 2]], min_pixels=10)
    out["two_buildings_same_plane"] = _shape([[0, 0, 1, 1]], [[1, 1, 1, 1]], min_pixels=10, merge_flat=True)
    out["two_buildings_other_planes"] = _shape([[0, 0, 1, 1]], [[1, 1, 2, 2]], zs=(100, 100), min_pixels=10, merge_flat=True)
    out["diagonal_only"] = _shape([[0, -1], [-1, 0]], [[1, 0], [0, 2]], min_pixels=5, merge_flat=True)
    for n in (65, 257, 4097):
        out[f"strip_{n}"] = strip(n)
    twin = [[1, 1, 2, 2]] * 2
    out["coplanar_merge_flat"] = _shape(np.zeros((2, 4)), twin, zs=(100, 100), merge_flat=True)
    out["coplanar_without_merge_flat"] = _shape(np.zeros((2, 4)), twin, zs=(100, 100), merge_flat=False)
    normal = np.array([[-1.0, 0.0, 1.0], [1.0, 0.0, 1.0]])
    center = np.array([[30, 0, 1030], [30, 0, 1030]])
    out["gable_is_a_ridge"] = _shape(np.zeros((3, 6)), [[1, 1, 1, 2, 2, 2]] * 3, normal=normal, center=center, merge_flat=True)
    out["step"] = _shape(np.zeros((2, 4)), twin, zs=(100, 1000), merge_flat=True, step_tol=200)
    out["checkerboard_8"] = checkerboard(8, 8)
    return out


def _speckle(rng, h, w, npl, size, p):
    roof = sc._patches(rng, h, w, npl, size) + 1
    return np.where(rng.random((h, w)) < p, rng.integers(-1, npl + 1, (h, w)), roof)


def _tables(rng, npl, w, h, bin, base, kind):
    """planes that coincide often: flat ones at two heights (FLAT and STEP edges), and sloped ones in equal pairs"""
    if kind == 0:
        normal = np.tile([0.0, 0.0, 1.0], (npl, 1))
        center = np.stack([np.zeros(npl), np.zeros(npl), base + 100 + 400 * rng.integers(0, 2, npl)], 1)
    else:
        normal, center = sc._planes(rng, npl, w, h, bin, base + 800, base + 1000, 0.3)
        for k in range(1, npl, 2):  # every second plane repeats the one before it
            normal[k], center[k] = normal[k - 1], center[k - 1]
    return normal, center


def small_case(seed):
    """at most 12 x 12, for the brute force"""
    rng = np.random.default_rng(21000 + seed)
    h, w = (int(v) for v in rng.integers(1, 13, 2))
    nb, npl = int(rng.integers(1, 4)), int(rng.integers(1, 6))
    bin, base = int(rng.choice([1, 10])), int(rng.integers(-5, 5))
    bmap = sc._patches(rng, h, w, nb + 1, 6) - (seed % 3 == 0)
    bmap = np.minimum(bmap, nb - 1)
    roof = _speckle(rng, h, w, npl, int(rng.integers(2, 5)), 0.25)
    normal, center = _tables(rng, npl, w, h, bin, base, seed % 2)
    c = sc.make(bmap, roof, nb, normal, center, np.full(npl, base), np.full(npl, base + 3000), bin, base,
                base + rng.integers(0, 600, nb))
    c["roof"] = np.where(c["bmap"] < 0, -1, roof).astype(np.int32)
    c["params"] = params(min_pixels=int(rng.choice([0, 1, 2, 3, 5, 20])), merge_flat=bool(rng.integers(0, 2)),
                         step_tol=int(rng.choice([0, 50, 200])), bend_tol=int(rng.choice([0, 4])),
                         max_rounds=int(rng.choice([0, 1, 2, 64, 64, 64])))
    return c


def fuzz_case(seed):
    """the cases of the device suite: up to 90 x 40, patches of planes with speckle, several buildings"""
    rng = np.random.default_rng(22000 + seed)
    w, h = int(rng.integers(20, 91)), int(rng.integers(10, 41))
    nb, npl = int(rng.integers(1, 5)), int(rng.integers(2, 8))
    bin, base = int(rng.choice([5, 10, 25])), int(rng.integers(-50, 50))
    bmap = np.minimum(sc._patches(rng, h, w, nb + 1, 25) - (seed % 2), nb - 1)
    roof = _speckle(rng, h, w, npl, int(rng.integers(4, 12)), float(rng.choice([0.03, 0.1, 0.3])))
    normal, center = _tables(rng, npl, w, h, bin, base, seed % 2)
    c = sc.make(bmap, roof, nb, normal, center, np.full(npl, base), np.full(npl, base + 3000), bin, base,
                base + rng.integers(0, 600, nb))
    c["roof"] = np.where(c["bmap"] < 0, -1, roof).astype(np.int32)
    c["params"] = params(min_pixels=int(rng.choice([0, 2, 4, 9, 30])), merge_flat=bool(seed % 3),
                         step_tol=int(rng.choice([0, 50, 200])), bend_tol=int(rng.choice([0, 4])))
    return c


def blob_case(w, h, seed):
    """the blob case of the solids at a given size, generalised with both rules"""
    c = sc.blob_case(w, h, seed, size=5, nb=6)
    c["params"] = params(min_pixels=6, merge_flat=True, step_tol=300)
    return c


def all_cases():
    for name, c in named_shapes().items():
        yield name, c
    for seed in range(N_FUZZ):
        yield f"fuzz_{seed}", fuzz_case(seed)
    yield "round_cap", with_params(fuzz_case(SEED_THREE_ROUNDS), max_rounds=1)
    yield "no_pixels", _shape(np.full((3, 4), -1), np.zeros((3, 4)), nb=0, min_pixels=3)
    yield "caps_above", caps_case(FIG_CAP + 1, PLANE_CAP + 1)
    yield "facet_over_seams_x", _shape(np.zeros((17, 65)), np.ones((17, 65)), min_pixels=2)
    yield "facet_over_seams_y", _shape(np.zeros((65, 17)), np.ones((65, 17)), min_pixels=2)


def regimes(c, ref=None):
    """the set of REGIMES the case reaches, from the restatement"""
    ref = run_ref(c) if ref is None else ref
    p = c["params"]
    bmap, roof0 = c["bmap"], c["roof"]
    h, w = bmap.shape
    out = set()
    inb = bmap >= 0
    if not inb.any():
        out.add("no_pixels")
    if (bmap[:, :-1] != bmap[:, 1:])[inb[:, :-1] & inb[:, 1:]].any() or (bmap[:-1] != bmap[1:])[inb[:-1] & inb[1:]].any():
        out.add("two_buildings_touch")
    if h > 1 and w > 1:
        d1 = (bmap[:-1, :-1] >= 0) & (bmap[:-1, :-1] == bmap[1:, 1:]) & (bmap[:-1, 1:] != bmap[:-1, :-1]) & (bmap[1:, :-1] != bmap[:-1, :-1])
        if d1.any():
            out.add("diagonal_contact")
    if inb.any():
        out.add("building_lds" if bmap.max() < FIG_CAP else "building_global")
        if bmap.min(where=inb, initial=FIG_CAP) < FIG_CAP:
            out.add("building_lds")
        pl = np.maximum(np.concatenate([roof0[inb], ref.roof[inb]]), 0)
        out.add("plane_lds" if pl.min() < PLANE_CAP else "plane_global")
        if pl.max() >= PLANE_CAP:
            out.add("plane_global")
    changed = ref.roof != roof0
    if ((roof0 <= 0) & inb & ~changed).any() and ref.rounds > 0:
        out.add("unroofed_value_kept")
    if ref.rounds >= 3:
        out.add("three_rounds")
    if not ref.converged:
        out.add("round_cap")
    first_flat_borders = None
    for r, ev in enumerate(ref.evals):
        rf = ev.rf
        nf = rf.n_facets
        if nf == 0:
            continue
        nbr = [[] for _ in range(nf)]
        for (lo, hi), ln in zip(rf.edge_facet.tolist(), rf.edge_length.tolist()):
            nbr[lo].append((hi, ln))
            nbr[hi].append((lo, ln))
        small = rf.facet_pixels < p["min_pixels"]
        for f in range(nf):
            if small[f] and not ev.moves[f]:
                if not nbr[f]:
                    out.add("stays_without_neighbour")
                elif all(rf.facet_plane[g] == 0 for g, _ in nbr[f]):
                    out.add("stays_unroofed_neighbour_only")
                elif r == 0 and changed[rf.facet == f].any():
                    out.add("waits_then_moves")
            if ev.moves[f]:
                out.add("moves_flat" if ev.by_flat[f] else "moves_small")
                if rf.facet_plane[f] == 0:
                    out.add("unroofed_moves")
                t = int(ev.target[f])
                ln = dict(nbr[f])[t]
                px = rf.facet_pixels
                if sum(1 for g, l in nbr[f] if l == ln and rf.facet_plane[g] > 0 and (px[g], -g) > (px[f], -f)) > 1:
                    out.add("length_tie")
        if ev.links.max() >= 2:
            out.add("chain_of_two")
        # pixel edges behind the FLAT moves of a later evaluation that lay on an edge of another kind in the first
        b = fr.border_edges(bmap, rf.facet.astype(np.int64), ev.top)
        ids = (b["y"] * w + b["x"]) * 2 + b["d"]
        key = np.minimum(b["fa"], b["fb"]) * nf + np.maximum(b["fa"], b["fb"])
        ekey = rf.edge_facet[:, 0].astype(np.int64) * nf + rf.edge_facet[:, 1]
        if r == 0:
            not_flat = ekey[ev.kind != 0]
            first_flat_borders = set(ids[np.isin(key, not_flat)].tolist())
        else:
            fm = np.nonzero(ev.by_flat)[0]
            used = np.minimum(fm, ev.target[fm]) * nf + np.maximum(fm, ev.target[fm])
            if first_flat_borders & set(ids[np.isin(key, used)].tolist()):
                out.add("flat_only_later")
    if w > 64 and (ref.evals[-1].rf.facet[:, 63] == ref.evals[-1].rf.facet[:, 64])[inb[:, 63] & inb[:, 64]].any():
        out.add("tile_seam_x")
    if h > 16 and (ref.evals[-1].rf.facet[15] == ref.evals[-1].rf.facet[16])[inb[15] & inb[16]].any():
        out.add("tile_seam_y")
    return out
