"""Cases for the roof facets (include/bs_api.h, "roof facets"): the inputs of tests/solid_ref/cases.py with the tops of
solid_ref.tops, the named shapes, fuzz cases of their own, and `regimes`: which rows of the threshold table (DESIGN.md,
"Roof facets") a case reaches, worked out from its inputs and the reference alone."""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "solid_ref"))
import facet_ref as fr  # noqa: E402
import solid_ref as sr  # noqa: E402


def _solid_cases():
    """tests/solid_ref/cases.py under a name of its own (this directory has a cases.py too)"""
    if "solid_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("solid_cases", os.path.join(HERE, "..", "solid_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["solid_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["solid_cases"]


sc = _solid_cases()

TW, TH = 64, 16  # the labelling tile of bs_facet.hip
N_SMALL, N_SOLID_FUZZ, N_FUZZ = 60, sc.N_FUZZ, 16
KIND_TOLS = (50, 0)  # step_tol, bend_tol of the kind rows
REGIMES = ("facet_single_pixel", "facet_unroofed", "facet_spans_tiles_x", "facet_spans_tiles_y", "tile_local_split",
           "facet_with_hole", "same_plane_two_facets", "diagonal_contact", "other_building_same_plane", "image_border",
           "edge_no_step", "edge_both_directions", "edge_in_pieces", "kind_flat", "kind_ridge", "kind_valley", "kind_step",
           "wave_uniform", "wave_mixed", "no_pixels", "many_facets")
# widths and heights around the tile, both orientations
SIZES = sorted({s for a in (1, TH - 1, TH, TH + 1, TW - 1, TW, TW + 1, 129, 257) for s in ((a, 33), (33, a))} |
               {(1, 1), (TW, TH), (TW + 1, TH + 1), (257, 129), (129, 257)})


def from_solid(c):
    """a solid case as a facet case: its map, its roof image and the tops the solids give it"""
    top = sr.tops(*[c[k] for k in sc.KEYS if k != "n_buildings"])
    return dict(bmap=c["bmap"], roof=c["roof"], top=top, n_buildings=c["n_buildings"], n_planes=len(c["z_min"]), bin=c["bin"],
                solid=c)


def run_ref(c):
    return fr.roof_facets(c["bmap"], c["roof"], c["top"])


def small_case(seed):
    return from_solid(sc.small_case(seed))


def solid_fuzz_case(seed):
    return from_solid(sc.fuzz_case(seed))


def blob_case(w, h, seed, size=9, nb=12):
    return from_solid(sc.blob_case(w, h, seed, size=size, nb=nb))


def fuzz_case(seed):
    """the facet fuzz cases: up to 200 x 60, so that facets cross tile seams in x and in y"""
    rng = np.random.default_rng(11000 + seed)
    kind = seed % 4
    w, h = int(rng.integers(60, 201)), int(rng.integers(14, 61))
    bin, base = int(rng.choice([5, 10, 25])), int(rng.integers(-50, 50))
    if kind == 0:  # large patches of few planes: facets wider and taller than a tile, flat planes at a few heights
        nb, npl = 3, 4
        bmap = sc._patches(rng, h, w, nb + 1, 45) - 1
        roof = sc._patches(rng, h, w, npl + 1, 23)
        normal = np.tile([0.0, 0.0, 1.0], (npl, 1))
        center = np.stack([np.zeros(npl), np.zeros(npl), base + 100 * rng.integers(1, 3, npl)], 1)
        return from_solid(sc.make(bmap, roof, nb, normal, center, np.full(npl, base), np.full(npl, base + 1000), bin, base,
                                  base + 100 * rng.integers(1, 3, nb)))
    if kind == 1:  # sloped planes in patches with noise pixels of other planes: holes, single pixels, diagonal contact
        nb, npl = 5, 6
        bmap = sc._patches(rng, h, w, nb + 2, 30) - 2
        roof = sc._patches(rng, h, w, npl, 12) + 1
        noise = rng.random((h, w)) < 0.08
        roof = np.where(noise, rng.integers(0, npl + 1, (h, w)), roof)
        normal, center = sc._planes(rng, npl, w, h, bin, base + 2000, base + 4000, 0.3)
        return from_solid(sc.make(bmap, roof, nb, normal, center, np.full(npl, base + 1500), np.full(npl, base + 5000), bin,
                                  base, base + rng.integers(0, 3000, nb)))
    if kind == 2:  # thin diagonal stripes of two planes over one building: long chains through many tiles
        yy, xx = np.mgrid[0:h, 0:w]
        period = int(rng.integers(3, 7))
        roof = 1 + ((xx + yy) // period) % 2
        roof = np.where(rng.random((h, w)) < 0.3, np.roll(roof, 1, axis=1), roof)
        bmap = np.where(rng.random((h, w)) < 0.02, -1, 0)
        normal, center = sc._planes(rng, 2, w, h, bin, base + 500, base + 600, 0.5)
        return from_solid(sc.make(bmap, roof, 1, normal, center, [base] * 2, [base + 2000] * 2, bin, base, [base + 300]))
    # kind 3: every pixel a plane of its own choice among three, two buildings side by side
    npl = 3
    bmap = (np.arange(w)[None, :] >= w // 2) * np.ones((h, 1), np.int64)
    roof = rng.integers(0, npl + 1, (h, w))
    normal, center = sc._planes(rng, npl, w, h, bin, base + 100, base + 200, 1.0)
    return from_solid(sc.make(bmap, roof, 2, normal, center, np.full(npl, base), np.full(npl, base + 400), bin, base,
                              [base + 100, base + 150]))


def _shape(bmap, roof, zs=(100, 200), normal=None, center=None, nb=None, bin=10):
    """a named shape: flat planes at the heights zs (or the tables given), clamps that never decide, base_z 0"""
    bmap = np.asarray(bmap)
    n = len(zs) if normal is None else len(normal)
    if normal is None:
        normal, center = np.tile([0.0, 0.0, 1.0], (n, 1)), np.stack([np.zeros(n), np.zeros(n), np.asarray(zs)], 1)
    nb = int(bmap.max()) + 1 if nb is None else nb
    return from_solid(sc.make(bmap, roof, nb, normal, center, np.full(n, -10 ** 6), np.full(n, 10 ** 6), bin, 0, np.full(nb, 50)))


def _gable(sign):
    """6 x 3 pixels of one building, bin 10: plane 1 over x < 3 and plane 2 over x >= 3 meet at X = 30 at equal height;
    sign +1: both rise towards the middle (a ridge), -1: both fall towards it (a valley)"""
    normal = np.array([[-1.0 * sign, 0.0, 1.0], [1.0 * sign, 0.0, 1.0]])
    center = np.array([[30, 0, 1030], [30, 0, 1030]])
    roof = np.array([[1, 1, 1, 2, 2, 2]] * 3)
    return _shape(np.zeros((3, 6)), roof, normal=normal, center=center)


def named_shapes():
    """name -> case: the shapes the tests name"""
    out = {}
    out["one_pixel"] = _shape([[0]], [[1]])
    out["two_pixels_one_plane"] = _shape([[0, 0]], [[1, 1]])
    out["two_pixels_diagonal"] = _shape([[0, -1], [-1, 0]], [[1, 0], [0, 1]])
    out["two_buildings_same_plane"] = _shape([[0, 1]], [[1, 1]])
    ring = np.ones((5, 5), np.int64)
    ring[2, 2] = 2
    out["ring_with_hole"] = _shape(np.zeros((5, 5)), ring)
    # a one-pixel-wide serpentine of plane 1 over 130 x 40: every even row, joined at alternating ends; the rest is plane 2
    serp = np.full((40, 130), 2, np.int64)
    serp[0::2, :] = 1
    serp[1::4, -1] = 1
    serp[3::4, 0] = 1
    out["serpentine"] = _shape(np.zeros((40, 130)), serp)
    # combs of plane 1 whose teeth join only through a spine beyond a tile seam
    comb = np.full((12, 80), 2, np.int64)
    comb[0::2, :TW + 7] = 1
    comb[:, TW + 6] = 1
    out["comb_x"] = _shape(np.zeros((12, 80)), comb)
    comb = np.full((TH + 8, 12), 2, np.int64)
    comb[:TH + 5, 0::2] = 1
    comb[TH + 4, :] = 1
    out["comb_y"] = _shape(np.zeros((TH + 8, 12)), comb)
    out["same_plane_two_pieces"] = _shape([[0, 0, 0]], [[1, 2, 1]])
    out["two_flat_planes_equal_height"] = _shape([[0, 0], [0, 0]], [[1, 2], [1, 2]], zs=(100, 100))
    out["gable"] = _gable(1)
    out["inverted_gable"] = _gable(-1)
    yy, xx = np.mgrid[0:8, 0:8]
    out["plane_checkerboard"] = _shape(np.zeros((8, 8)), 1 + (yy + xx) % 2, zs=(100, 600))
    return out


def all_cases():
    """(name, case) of everything the regime test looks at: the named shapes, the solid fuzz cases, the facet fuzz cases"""
    for name, c in named_shapes().items():
        yield name, c
    for seed in range(N_SOLID_FUZZ):
        yield f"solid_fuzz_{seed}", solid_fuzz_case(seed)
    for seed in range(N_FUZZ):
        yield f"fuzz_{seed}", fuzz_case(seed)


def _has_hole(mask):
    """a 4-connected set of pixels has a hole iff its complement (8-connected, the outside included) is not one piece"""
    pad = np.pad(~mask, 1, constant_values=True)
    return ndimage.label(pad, structure=np.ones((3, 3)))[1] > 1


def regimes(c, ref=None):
    """the rows of REGIMES this case reaches"""
    bmap, roof, top = np.asarray(c["bmap"], np.int64), np.asarray(c["roof"], np.int64), c["top"]
    h, w = bmap.shape
    inb = bmap >= 0
    if not inb.any():
        return {"no_pixels"}
    r = run_ref(c) if ref is None else ref
    facet = r.facet.astype(np.int64)
    out = set()
    if (r.facet_pixels == 1).any():
        out.add("facet_single_pixel")
    if (r.facet_plane == 0).any():
        out.add("facet_unroofed")
    bb = r.facet_bbox.astype(np.int64)
    if (bb[:, 0] // TW != bb[:, 2] // TW).any():
        out.add("facet_spans_tiles_x")
    if (bb[:, 1] // TH != bb[:, 3] // TH).any():
        out.add("facet_spans_tiles_y")
    # tile-local components: only the links inside a tile count
    cls = fr.classes(bmap, roof)
    local = fr.components(cls, keep_h=(np.arange(1, w) % TW != 0)[None, :], keep_v=(np.arange(1, h) % TH != 0)[:, None])
    ys, xs = np.nonzero(inb)
    tile = (ys // TH) * (w // TW + 1) + xs // TW
    ft = np.unique(np.stack([facet[ys, xs], tile, local[ys, xs]], 1), axis=0)  # distinct (facet, tile, local component)
    _, per = np.unique(ft[:, :2], axis=0, return_counts=True)
    if (per > 1).any():
        out.add("tile_local_split")
    for f in np.nonzero(r.facet_pixels >= 8)[0]:
        x0, y0, x1, y1 = bb[f]
        if x1 - x0 >= 2 and y1 - y0 >= 2 and _has_hole(facet[y0:y1 + 1, x0:x1 + 1] == f):
            out.add("facet_with_hole")
            break
    if len(np.unique(np.stack([r.facet_building, r.facet_plane], 1), axis=0)) < r.n_facets:
        out.add("same_plane_two_facets")
    for a, b in (((slice(None, -1), slice(None, -1)), (slice(1, None), slice(1, None))),
                 ((slice(None, -1), slice(1, None)), (slice(1, None), slice(None, -1)))):
        if ((cls[a] >= 0) & (cls[a] == cls[b]) & (facet[a] != facet[b])).any():
            out.add("diagonal_contact")
    P = np.maximum(roof, 0)
    for a, b in (((slice(None), slice(None, -1)), (slice(None), slice(1, None))),
                 ((slice(None, -1), slice(None)), (slice(1, None), slice(None)))):
        if ((bmap[a] >= 0) & (bmap[b] >= 0) & (bmap[a] != bmap[b]) & (P[a] == P[b])).any():
            out.add("other_building_same_plane")
    if inb[0].any() or inb[-1].any() or inb[:, 0].any() or inb[:, -1].any():
        out.add("image_border")
    if (r.edge_n_step == 0).any():
        out.add("edge_no_step")
    if ((r.edge_n_dir0 > 0) & (r.edge_n_dir0 < r.edge_length)).any():
        out.add("edge_both_directions")
    if r.n_border:  # an edge in pieces: its border edges, joined where they share a lattice corner, are not one piece
        b = fr.border_edges(bmap, facet, top)
        nf = r.n_facets
        pairs = r.edge_facet.astype(np.int64)
        e = np.searchsorted(pairs[:, 0] * nf + pairs[:, 1], np.minimum(b["fa"], b["fb"]) * nf + np.maximum(b["fa"], b["fb"]))
        nc = (w + 1) * (h + 1)
        s, t = e * nc + b["sy"] * (w + 1) + b["sx"], e * nc + b["ey"] * (w + 1) + b["ex"]
        nodes, inv = np.unique(np.concatenate([s, t]), return_inverse=True)
        inv = inv.reshape(-1)
        g = fr.coo_matrix((np.ones(len(s), np.int8), (inv[:len(s)], inv[len(s):])), shape=(len(nodes), len(nodes)))
        comp = fr.connected_components(g, directed=False)[1]
        pieces = np.unique(np.stack([nodes // nc, comp], 1), axis=0)
        if len(pieces) > r.n_edges:
            out.add("edge_in_pieces")
    kinds = fr.kinds(r, *KIND_TOLS)
    for k, name in enumerate(("kind_flat", "kind_ridge", "kind_valley", "kind_step")):
        if (kinds == k).any():
            out.add(name)
    flat = facet.ravel()
    flat = np.concatenate([flat, np.full(-len(flat) % 64, -1)]).reshape(-1, 64)
    uni = (flat == flat[:, :1]).all(1)
    if (uni & (flat[:, 0] >= 0)).any():
        out.add("wave_uniform")
    if (~uni).any():
        out.add("wave_mixed")
    if 2 * r.n_facets >= r.n_pixels:
        out.add("many_facets")
    assert out <= set(REGIMES), out - set(REGIMES)
    return out
