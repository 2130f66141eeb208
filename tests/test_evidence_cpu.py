"""Roof evidence without a GPU (include/bs_api.h, "plane quality", "roof evidence", "footprint screen"): the names in the
header and the loader; the numpy restatement against the brute force of the definition, every image and figure with ==; the
errors of the definition; bs_plane_quality (host only) on a hand-made table; and the premise on the boxes with trees: what
today's chain makes of a tree, what the quality rule tells apart, and what the default screen finds."""
import ctypes as C
import importlib.util
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_plane_quality", "bs_roof_evidence_dev", "bs_roof_evidence", "bs_set_footprint_screen", "bs_set_footprint_screen_dev",
       "bs_get_footprint_screen"]


def load_evidence_cases():
    if "evidence_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("evidence_cases", os.path.join(HERE, "evidence_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["evidence_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["evidence_cases"]


cases = load_evidence_cases()
eref, brute, gref = cases.eref, cases.brute, cases.gref
BY_NAME = cases.BY_NAME
_REF = {}


def ref(name):
    """the restatement's result, computed once and never changed"""
    if name not in _REF:
        _REF[name] = eref.evidence(*cases.args(BY_NAME[name]))
    return _REF[name]


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(os.path.dirname(HERE), "include", "bs_api.h")).read()
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    for name in ("roof_evidence", "roof_evidence_dev", "set_footprint_screen", "footprint_screen"):
        assert callable(getattr(api.Context, name))
    assert api.RoofEvidence and callable(api.evidence_params) and callable(api.plane_quality)
    for k, v in (("BS_EVIDENCE_RMAX", _lib.EVIDENCE_RMAX), ("BS_EVIDENCE_TILE", _lib.EVIDENCE_TILE),
                 ("BS_EVIDENCE_GRID", _lib.EVIDENCE_GRID)):
        assert int(re.search(r"#define %s\s+(\d+)" % k, txt).group(1)) == v
    assert (cases.TILE, cases.GRID, brute.RMAX) == (_lib.EVIDENCE_TILE, _lib.EVIDENCE_GRID, _lib.EVIDENCE_RMAX)
    assert C.sizeof(_lib.RoofEvidence) == 4 * 10 + 8 * 7 + 8 * 2
    assert int(re.search(r"#define BS_API_VERSION (\d+)", txt).group(1)) == 5 == L.bs_api_version()


def test_default_parameters():
    p = api.evidence_params()
    assert p == dict(r=3, min_points=1, num=1, den=2, min_plane_points=0, max_rms_mm=100)
    assert {k: p[k] for k in ("r", "min_points", "num", "den")} == brute.params()
    assert api.evidence_params(r=0, share=(2, 3), max_rms_mm=50)["den"] == 3


@pytest.mark.parametrize("name", [c["name"] for c in cases.CASES])
def test_restatement_equals_brute_force(name):
    assert eref.same(ref(name), brute.evidence(*cases.args(BY_NAME[name]))) is None


def test_what_the_cases_are_there_for():
    r = ref("one_point")
    assert (r.width, r.height, r.n_counted, r.n_planar, r.pixels_kept) == (2, 2, 1, 1, 1) and r.keep[0, 0] == 1
    r = ref("r0")
    assert np.array_equal(r.win_above, r.above) and r.pixels_rejected > 0 < r.pixels_kept
    assert 2 * 15 + 1 > ref("r15_narrow").width and ref("r15_narrow").pixels_rejected > 0 < ref("r15_narrow").pixels_kept
    r = ref("straddle_small")
    assert r.width > cases.TILE < r.height and r.win_above[cases.TILE, cases.TILE] > 0
    r = ref("no_planes")
    assert r.n_planar == 0 < r.n_counted and r.pixels_kept == 0 < r.pixels_rejected
    assert ref("every_plane").n_planar > ref("every_plane").n_counted // 2
    r = ref("num_zero")
    assert r.pixels_rejected == 0 and r.pixels_kept == int((r.win_above > 0).sum())
    r = ref("num_is_den")
    assert (r.keep[1, 1], r.keep[1, 4], r.pixels_kept, r.pixels_rejected) == (1, 0, 1, 1)
    r = ref("all_below")
    assert r.n_counted == 0 and not r.keep.any() and (r.pixels_kept, r.pixels_rejected, r.pixels_thin, r.max_window) == (0, 0, 0, 0)
    r = ref("labels")  # of five counting points, only the one of plane 1 is planar
    assert (r.n_counted, r.n_planar) == (5, 1) and r.keep[1].tolist() == [0, 0, 0, 0, 1, 0, 0, 0]
    r = ref("share_boundary")
    (xk, yk), (xd, yd) = cases.BOUNDARY_KEPT, cases.BOUNDARY_DROPPED
    assert (r.win_above[yk, xk], r.win_planar[yk, xk], r.keep[yk, xk]) == (4, 2, 1)
    assert (r.win_above[yd, xd], r.win_planar[yd, xd], r.keep[yd, xd]) == (5, 2, 0)
    x, y = cases.THIN_AT
    a, b = ref("min_points_at"), ref("min_points_over")
    assert a.win_above[y, x] == 3 and a.keep[y, x] == 1 and (a.pixels_kept, a.pixels_thin) == (9, 0)
    assert b.win_above[y, x] == 3 and b.keep[y, x] == 0 and (b.pixels_kept, b.pixels_thin) == (0, 9)
    # the model: its rule differs from the scalar's, one entry is EMPTY and some points lie beyond the table
    c = BY_NAME["model"]
    dtm, cell, _ = c["model"]
    q = c["xyz"].astype(np.int64)
    assert (gref.below(q, c["ground_th"], c["model"]) != gref.below(q, c["ground_th"])).sum() > 50
    assert (q[:, 0] // cell >= dtm.shape[1]).sum() > 20 and (dtm == cases.EMPTY).sum() == 1
    gy, gx = np.argwhere(dtm == cases.EMPTY)[0]
    assert ((q[:, 0] // cell == gx) & (q[:, 1] // cell == gy)).any()
    big = {c["name"]: c for c in cases.large()}
    # more points than one sweep of the counts pass; every second point of a thread lies in the scan-ordered tail, in runs of
    # equal pixels that hold points below ground and points of rejected planes, and the last wave is partly idle
    c = big["sweep_points"]
    n, sweep = len(c["xyz"]), 256 * _lib.GROUND_GRID
    assert n > sweep == cases.SWEEP and n - cases.SWEEP_SCAN_TAIL < sweep and (n - sweep) % 64 != 0
    pix = (c["xyz"][sweep:, 1] // c["bin"]).astype(np.int64) * w40(c) + c["xyz"][sweep:, 0] // c["bin"]
    runs = np.diff(np.flatnonzero(np.diff(pix, prepend=-1, append=-1)))
    assert (np.diff(pix) >= 0).all() and len(runs) > 100 and np.median(runs) >= 16
    low, lab = c["xyz"][sweep:, 2] < c["ground_th"], c["plane_idx"][sweep:]
    assert low.sum() > 1000 < (~low).sum() and (lab == 2).sum() > 1000 < (lab == 1).sum() and c["plane_ok"].tolist() == [1, 0, 1, 1, 0]
    s = BY_NAME["scan_order"]
    pix = (s["xyz"][:, 1] // 100).astype(np.int64) * 20 + s["xyz"][:, 0] // 100
    assert (np.diff(pix) >= 0).all() and 8 <= len(np.unique(pix[:64])) <= 32  # several runs in the first wave
    w, h = brute.grid_dims(big["sweep_pixels"]["extent"], 100)
    assert -(-w // cases.TILE) * -(-h // cases.TILE) > cases.GRID


def w40(c):
    return brute.grid_dims(c["extent"], c["bin"])[0]


def test_errors_of_the_definition():
    c = BY_NAME["r1"]
    base = dict(zip(("xyz", "plane_idx", "n_planes", "plane_ok", "extent", "bin", "ground_th", "params", "model"), cases.args(c)))

    def both(exc, **kw):
        a = dict(base, **kw)
        for fn in (eref.evidence, brute.evidence):
            with pytest.raises(exc):
                fn(*[a[k] for k in base])

    def moved(axis, value):
        q = c["xyz"].copy()
        q[5, axis] = value
        return q
    p = c["params"]
    both(brute.InvalidError, xyz=c["xyz"][:0], plane_idx=c["plane_idx"][:0])
    both(brute.InvalidError, bin=0)
    both(brute.InvalidError, n_planes=-1, plane_ok=None)
    both(brute.InvalidError, extent=np.array([-1, 5, 0]))
    for kw in (dict(r=-1), dict(r=16), dict(min_points=0), dict(den=0), dict(num=-1), dict(num=3, den=2)):
        both(brute.InvalidError, params=dict(p, **kw))
    w, h = brute.grid_dims(c["extent"], c["bin"])
    both(brute.RangeError, xyz=moved(0, -1))
    both(brute.RangeError, xyz=moved(1, -1))
    both(brute.RangeError, xyz=moved(0, w * c["bin"]))
    both(brute.RangeError, xyz=moved(1, h * c["bin"]))
    both(brute.RangeError, extent=np.array([2 ** 31 - 1, 2 ** 31 - 1, 0]), bin=1)
    ok = moved(0, w * c["bin"] - 1)  # the last pixel of a row is inside
    a = dict(base, xyz=ok)
    assert eref.same(eref.evidence(*[a[k] for k in base]), brute.evidence(*[a[k] for k in base])) is None


# ---- bs_plane_quality: host only --------------------------------------------------------------------------------------------
def test_plane_quality_on_a_hand_made_table():
    n = 1000
    limit = 100 * 100 * n
    rows = [(0, n, limit), (0, n, limit + 1), (1, n, 0), (2, n, 0), (0, n, 0), (0, n + 1, 0), (0, 0, 0), (0, 3, 3 * 10000)]
    fits = SimpleNamespace(n_planes=len(rows), status=np.array([r[0] for r in rows], np.int32),
                           n_points=np.array([r[1] for r in rows], np.int64), r_sq_sum=np.array([r[2] for r in rows], np.int64))
    # the rms exactly at the limit is kept, one unit over it is dropped, status 1 and 2 are dropped
    assert api.plane_quality(fits).tolist() == [1, 0, 0, 0, 1, 1, 1, 1]
    # min_points at n and n + 1
    assert api.plane_quality(fits, min_points=n).tolist() == [1, 0, 0, 0, 1, 1, 0, 0]
    assert api.plane_quality(fits, min_points=n + 1).tolist() == [0, 0, 0, 0, 0, 1, 0, 0]
    assert api.plane_quality(fits, max_rms_mm=0).tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    for kw in (dict(), dict(min_points=n), dict(min_points=n + 1), dict(max_rms_mm=0), dict(max_rms_mm=32767)):
        want = eref.plane_quality(fits.status, fits.n_points, fits.r_sq_sum, kw.get("min_points", 0), kw.get("max_rms_mm", 100))
        assert np.array_equal(api.plane_quality(fits, **kw), want), kw
    # 32767^2 * 2^29 and the largest r_sq_sum stay exact
    wide = SimpleNamespace(n_planes=2, status=np.zeros(2, np.int32), n_points=np.array([2 ** 29 - 1] * 2, np.int64),
                           r_sq_sum=np.array([32767 ** 2 * (2 ** 29 - 1), 2 ** 63 - 1], np.int64))
    assert api.plane_quality(wide, max_rms_mm=32767).tolist() == [1, 0]
    for kw in (dict(min_points=-1), dict(max_rms_mm=-1), dict(max_rms_mm=32768)):
        with pytest.raises(api.BsError):
            api.plane_quality(fits, **kw)
        with pytest.raises(brute.InvalidError):
            eref.plane_quality(fits.status, fits.n_points, fits.r_sq_sum, kw.get("min_points", 0), kw.get("max_rms_mm", 100))
    L = _lib.load()
    ok = np.zeros(8, np.uint8)
    assert L.bs_plane_quality(None, 0, 100, ok.ctypes.data) == -1
    f = _lib.PlaneFits()
    f.n_planes = 3  # null arrays with n_planes > 0
    assert L.bs_plane_quality(C.byref(f), 0, 100, ok.ctypes.data) == -1
    f.n_planes = 0
    assert L.bs_plane_quality(C.byref(f), 0, 100, None) == 0
    empty = SimpleNamespace(n_planes=0, status=np.zeros(0, np.int32), n_points=np.zeros(0, np.int64), r_sq_sum=np.zeros(0, np.int64))
    assert api.plane_quality(empty).shape == (0,)


# ---- the premise: boxes and trees -----------------------------------------------------------------------------------------
_PREMISE = {}


def premise(oracle, rise):
    """the tree scene, its labels from the oracle, the fit and the quality of its planes, the ground rule (on a slope: the
    ground model of tests/ground_ref at its defaults), and the reference chain without the screen, with the quality rule alone
    (r = 0) and with the default screen; computed once"""
    if rise not in _PREMISE:
        xyz, tree = cases.tree_scene(rise)
        neigh, normals = oracle.knn_normals(xyz, k=15)
        labels, planes = oracle.region_grow(xyz, normals, neigh)
        n_planes = len(planes["id"])
        status, n_points, r_sq = eref.plane_fit_figures(xyz, labels, n_planes)
        s = SimpleNamespace(xyz=xyz, tree=tree, labels=labels, n_planes=n_planes, rms=eref.rms(n_points, r_sq),
                            ok=eref.plane_quality(status, n_points, r_sq), th=gref.ground_th(xyz), model=None, truth=cases.truth_map())
        s.tree_share = np.array([tree[labels == p + 1].mean() for p in range(n_planes)])
        if rise:
            gp = gref.params()
            s.model = (gref.ground(xyz, xyz.max(0), gp).dtm, gp["cell"], gp["min_height"])
        s.plain = eref.building_chain(xyz, s.th, s.model)[1]
        for name, r in (("quality", 0), ("screen", 3)):
            e = eref.evidence(xyz, labels, n_planes, s.ok, xyz.max(0), cases.BIN, s.th, eref.params(r=r), s.model)
            setattr(s, name, SimpleNamespace(evidence=e, buildings=eref.building_chain(xyz, s.th, s.model, e.keep)[1]))
        _PREMISE[rise] = s
    return _PREMISE[rise]


def outside_share(bmap, truth):
    """per building: the share of its pixels outside the truth map"""
    return [float(((bmap == b) & (truth < 0)).sum()) / float((bmap == b).sum()) for b in range(int(bmap.max()) + 1)]


def check_premise(s, what):
    """the three conditions, the same for every scene: (a) without the screen a tree is a building and a box is lost; (b)
    max_rms_mm = 100 separates every tree plane (more than half of its points are tree points) from every real one; (c) the
    default screen finds exactly the boxes"""
    boxes = int(s.truth.max()) + 1
    assert s.plain.map.shape == s.truth.shape
    assert (s.tree_share > 0.5).sum() >= 3 and (s.tree_share <= 0.5).sum() >= 4
    on_plane = (s.labels >= 1) & (s.labels <= s.n_planes)
    assert on_plane[s.tree].sum() > s.tree.sum() // 2  # a label alone does not help: most tree points carry one
    plain = gref.box_scores(s.plain.map, s.truth)
    print(f"{what}: no screen: buildings {s.plain.n_buildings}, IoU {plain}")
    assert s.plain.n_buildings > boxes and min(plain) < 0.7                                     # (a)
    real, trees = s.rms[s.tree_share <= 0.5], s.rms[s.tree_share > 0.5]
    print(f"{what}: {s.n_planes} planes; rms of the {len(real)} real planes {np.sort(real).round(1).tolist()}, of the {len(trees)} "
          f"tree planes {np.sort(trees).round(1).tolist()}; {int(on_plane[s.tree].sum())} of {int(s.tree.sum())} tree points "
          f"carry a label")
    assert real.max() < 100 < trees.min()                                                        # (b)
    assert np.array_equal(s.ok != 0, s.tree_share <= 0.5)
    b = s.screen.buildings
    scores, out = gref.box_scores(b.map, s.truth), outside_share(b.map, s.truth)
    e = s.screen.evidence
    print(f"{what}: default screen: buildings {b.n_buildings}, IoU {scores}, outside {out}, kept {e.pixels_kept}, rejected "
          f"{e.pixels_rejected}, counted {e.n_counted}, planar {e.n_planar}")
    assert b.n_buildings == boxes and min(scores) >= 0.95 and max(out) <= 0.5                  # (c)
    # the quality rule alone, without a window (r = 0): the trees are gone but specks survive, which is why r = 3 is the default
    q = s.quality.buildings
    sizes = np.bincount(q.map[q.map >= 0])
    print(f"{what}: r = 0: buildings {q.n_buildings}, pixels of the smallest {np.sort(sizes)[:8].tolist()}, IoU "
          f"{gref.box_scores(q.map, s.truth)}")
    assert q.n_buildings >= boxes


def test_premise_level(oracle):
    """the level scene under the scalar rule: (a), (b) and (c)"""
    s = premise(oracle, 0)
    assert s.model is None
    check_premise(s, "level")


def test_premise_under_a_ground_model(oracle):
    """the same three conditions on the 10 % slope under the ground model of tests/ground_ref at its defaults (cell 500,
    min_height 2 000): the two switches compose"""
    s = premise(oracle, 100)
    assert s.model is not None and (s.model[1], s.model[2]) == (gref.params()["cell"], gref.params()["min_height"]) == (500, 2000)
    assert (gref.below(s.xyz, s.th, s.model) != gref.below(s.xyz, s.th)).sum() > 1000  # the model decides, not the scalar
    check_premise(s, "slope 100 under the model")
