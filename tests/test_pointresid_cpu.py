"""Point residuals without a GPU (include/bs_api.h, "point residuals"): the numpy restatement of the device layout against
the brute force of the definition (every point against every triangle, Python integers), every per-point value and figure
with ==; the four promises; the regimes of the threshold table; and the names in the header and the loader."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_modelraster_cpu import BY_NAME as MR_BY_NAME, ref as mr_ref, upstream as mr_upstream  # noqa: E402
from test_modelraster_cpu import uref, tref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_point_residuals_dev", "bs_point_residuals", "bs_point_residuals_free"]
# A run of up to BRUTE_PAIRS (point, triangle) pairs is compared whole with the brute force; a larger one on
# BRUTE_PAIRS / triangles points drawn by a fixed seed, beside every point that is not covered exactly once.
BRUTE_PAIRS = 200_000


def load_pointresid_cases():
    if "pointresid_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("pointresid_cases", os.path.join(HERE, "pointresid_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["pointresid_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["pointresid_cases"]


cases = load_pointresid_cases()
pref, brute, mref = cases.pref, cases.brute, cases.mref
OWN = cases.own_shapes()
BY_NAME = {}  # name -> (case, tolerances, bin)
for _name, _c, _tol, _bin in cases.all_runs():
    BY_NAME.setdefault(_name, (_c, [], _bin))[1].append(_tol)
_UP, _CLOUD, _REF = {}, {}, {}
# the NO_BRIDGE run of the triangle cases
(NB_NAME, NB_TOL, NB_LABEL), = cases.tc.NO_BRIDGE_RUNS
MUST_BE_WHOLE = (("bay", (100, 1)), ("staircase", (1, 1)), ("nested", (2, 1)), (NB_NAME, NB_TOL))


def upstream(name, tol):
    """(plain, clean, triangles) of the restatements of the stages before, computed once and never changed"""
    if name in MR_BY_NAME:
        return mr_upstream(name, tol)
    if (name, tol) not in _UP:
        c = BY_NAME[name][0]
        plain, _, clean = uref.clean(c["label"], c["top"], c["n_labels"], *tol)
        _UP[name, tol] = (plain, clean, tref.triangulate(plain, clean))
    return _UP[name, tol]


def cloud(name, tol, n_random=None):
    """the seeded cloud of a run, computed once and never changed"""
    if (name, tol, n_random) not in _CLOUD:
        c, _, b = BY_NAME[name]
        _, clean, tri = upstream(name, tol)
        _CLOUD[name, tol, n_random] = cases.cloud(name, c, tol, b, clean, tri, n_random)
    return _CLOUD[name, tol, n_random]


def ref(name, tol, n_random=None):
    """(the restatement's result on the run's cloud, its trace), computed once and never changed"""
    if (name, tol, n_random) not in _REF:
        c = BY_NAME[name][0]
        h, w = c["label"].shape
        _, clean, tri = upstream(name, tol)
        k = cloud(name, tol, n_random)
        trace = {}
        _REF[name, tol, n_random] = (pref.point_residuals(clean, tri, c["n_labels"], w, h, k.xyz, k.bin, k.plane_idx,
                                                          k.label_plane, k.clip2, trace), trace)
    return _REF[name, tol, n_random]


def against_brute(a, clean, tri, c, k):
    """True iff the run was compared whole"""
    h, w = c["label"].shape
    nt = max(int(tri.n_triangles), 1)
    if len(k.xyz) * nt <= BRUTE_PAIRS:
        b = brute.point_residuals(clean, tri, c["n_labels"], w, h, k.xyz, k.bin, k.plane_idx, k.label_plane, k.clip2)
        assert brute.same(a, b) is None, brute.same(a, b)
        return True
    rng = np.random.default_rng(len(k.xyz))
    n = max(BRUTE_PAIRS // nt, 16)
    odd = np.flatnonzero(a.cover != 1)
    odd = odd if len(odd) <= n else rng.choice(odd, n, replace=False)
    at = np.unique(np.concatenate([rng.integers(0, len(k.xyz), n), odd]))
    got = brute.sample(clean, tri, c["n_labels"], k.bin, k.xyz[at].tolist())
    assert got == list(zip(a.cover[at].tolist(), a.label[at].tolist(), a.r2[at].tolist()))
    return False


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert re.search(r"^struct bs_point_residuals \{", txt, flags=re.M)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("point_residuals", "point_residuals_dev", "point_fidelity"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "PointResiduals") and hasattr(api, "PointFidelity") and hasattr(api, "point_fidelity_of")
    assert L.bs_api_version() == 5
    for macro, mine, refs in (("FIG_CAP", _lib.PRESID_FIG_CAP, pref.FIG_CAP), ("CHUNK", _lib.PRESID_CHUNK, pref.CHUNK),
                              ("GRID", _lib.PRESID_GRID, pref.GRID)):
        v, = re.findall(r"^#define BS_PRESID_%s (\d+)" % macro, txt, flags=re.M)
        assert int(v) == mine == refs, macro
    # the struct of the loader follows the header field for field
    body = re.search(r"^struct bs_point_residuals \{(.*?)^\};", txt, flags=re.M | re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.PointResiduals._fields_]
    assert api.NO_CLIP2 == brute.NO_CLIP2


_WHOLE = set()


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_references_agree_and_promises_hold(name):
    """on every run: the restatement of the layout equals the brute force of the definition in every per-point value and
    figure, and the first three promises hold (at tolerance 0 every point gets the label of its base pixel)"""
    c = BY_NAME[name][0]
    for tol in BY_NAME[name][1]:
        a = ref(name, tol)[0]
        _, clean, tri = upstream(name, tol)
        k = cloud(name, tol)
        if against_brute(a, clean, tri, c, k):
            _WHOLE.add((name, tol))
        promised = brute.check_promises(a, c["label"], tri.label_status, tolerance_zero=tol[0] == 0, xyz=k.xyz)
        assert promised == (tol[0] == 0)
        if tol[0] == 0:
            assert a.n_multi == 0


def test_the_named_runs_were_compared_whole():
    """the cap of the brute force cannot empty the comparison: the bay, the staircase with its tie points, nested and the
    NO_BRIDGE run are compared whole, and the tie sets are not empty"""
    for name, tol in MUST_BE_WHOLE:
        if (name, tol) not in _WHOLE:
            test_references_agree_and_promises_hold(name)
        assert (name, tol) in _WHOLE, (name, tol)
    assert cloud("staircase", (1, 1)).n_ties >= 8 and cloud("bay", (100, 1)).n_ties > 0


@pytest.mark.parametrize("name", ["bay", "staircase", "nested", "band", "wide", NB_NAME, "pstrip_257"])
def test_bin_1_equals_the_model_raster(name):
    """the fourth promise: at bin 1 with one point per pixel in raster order, M, cover and mz2 are the three images of the
    model raster's restatement on the same triangles"""
    c = BY_NAME[name][0]
    h, w = c["label"].shape
    for tol in BY_NAME[name][1]:
        _, clean, tri = upstream(name, tol)
        xyz = cases.raster_cloud(c)
        r = pref.point_residuals(clean, tri, c["n_labels"], w, h, xyz, 1)
        m = mr_ref(name, tol)[0] if name in MR_BY_NAME else mref.model_raster(clean, tri, c["label"], c["top"], c["n_labels"])
        assert np.array_equal(r.label.reshape(h, w), m.model) and np.array_equal(r.cover.reshape(h, w), m.cover)
        mz2 = np.where(r.label >= 0, 2 * xyz[:, 2].astype(np.int64) - r.r2, brute.INT32_MIN)
        assert np.array_equal(mz2.reshape(h, w), m.mz2)
        assert r.n_rows == m.n_rows  # (the rows are the model raster's; the spans are wider: whole pixels of the band)


def test_every_regime_is_reached():
    """the rows of the threshold table ("Point residuals"), worked out from the references"""
    reached = {}
    for name, (c, tols, _) in BY_NAME.items():
        if name.startswith(("fuzz_", "line_", "random_")) and name not in ("random_0", "fuzz_1"):
            continue  # (what they reach the shapes reach too: the refs of the rest are enough for this test)
        for tol in tols:
            r, trace = ref(name, tol)
            for k in cases.regimes(upstream(name, tol)[2], r, trace):
                reached.setdefault(k, (name, tol))
    assert sorted(reached) == sorted(cases.REGIMES), sorted(set(cases.REGIMES) - set(reached))
    print(reached)


def test_shapes_are_what_they_are_for():
    r, trace = ref("staircase", (1, 1))
    assert trace["tie_owned"] > 0 and trace["tie_not_owned"] > 0 and r.n_multi == 0
    b = ref("bay", (100, 1))[0]
    assert b.n_multi > 0 and b.n_uncovered > 0 and b.multi.tolist()[1] == 0
    f = ref(NB_NAME, NB_TOL)[0]
    _, _, tri = upstream(NB_NAME, NB_TOL)
    assert tri.label_status[NB_LABEL] == cases.tbrute.NO_BRIDGE and f.points[NB_LABEL] == 0 and f.n_uncovered > 0
    d = ref("band", (2, 1))[0]
    assert d.max_list > 1 and d.n_empty_pixel > 0 and d.n_rows > 1000
    assert ref("wide", (0, 1))[1]["max_span"] > pref.CHUNK
    for n in cases.STRIPS:
        s = ref(f"pstrip_{n}", (0, 1))[0]
        assert s.n_labels == n and (s.points >= 1).all() and s.n_triangles == 2 * n and s.n_uncovered == 0
    w, nar = ref("slope_wide", (0, 1))[0], ref("slope_narrow", (0, 1))[0]
    assert w.n_height_wide == w.total_points == w.n_points and w.n_triangles == 2
    assert nar.n_height_wide == 0 and nar.total_points == nar.n_points
    _, clean, _ = upstream("slope_wide", (0, 1))
    assert int(np.min(clean.sz)) == -cases.Z_MAX and int(np.max(clean.sz)) == cases.Z_MAX


def test_ranges_and_arguments_of_the_definition():
    """both references refuse what the definition refuses"""
    c, _, b = BY_NAME["bay"]
    h, w = c["label"].shape
    _, clean, tri = upstream("bay", (0, 1))
    k = cloud("bay", (0, 1))

    def both(exc, xyz=k.xyz, bin=b, plane_idx=None, label_plane=None, clip2=0, clean=clean, width=w, height=h):
        for f in (pref.point_residuals, brute.point_residuals):
            with pytest.raises(exc):
                f(clean, tri, c["n_labels"], width, height, xyz, bin, plane_idx, label_plane, clip2)

    def moved(col, v):
        x = k.xyz.copy()
        x[3, col] = v
        return x

    both(brute.InvalidError, xyz=k.xyz[:0])
    both(brute.InvalidError, bin=0)
    both(brute.InvalidError, clip2=-1)
    both(brute.InvalidError, plane_idx=k.plane_idx)
    both(brute.InvalidError, label_plane=k.label_plane)
    both(brute.RangeError, xyz=moved(0, -1))
    both(brute.RangeError, xyz=moved(1, -1))
    both(brute.RangeError, xyz=moved(0, w * b))
    both(brute.RangeError, xyz=moved(1, h * b))
    both(brute.RangeError, xyz=moved(2, 1 << 24))
    both(brute.RangeError, xyz=moved(2, -(1 << 24)))
    both(brute.RangeError, bin=(1 << 24) // w + 1)
    from types import SimpleNamespace
    high = SimpleNamespace(sxy=clean.sxy, sz=np.full_like(np.asarray(clean.sz), 1 << 24))
    both(brute.RangeError, clean=high)
    ok = moved(2, (1 << 24) - 1)  # the largest height is inside
    assert brute.same(pref.point_residuals(clean, tri, c["n_labels"], w, h, ok, b),
                      brute.point_residuals(clean, tri, c["n_labels"], w, h, ok, b)) is None


def test_fidelity_by_building():
    """point_fidelity_of adds the per-label figures up by building"""
    r = ref("bay", (100, 1))[0]
    f = api.point_fidelity_of(r, [0, 1], 2)
    assert f.points.tolist() == r.points.tolist() and f.in_points.tolist() == r.in_points.tolist()
    one = api.point_fidelity_of(r, [0, 0])
    assert one.n_buildings == 1 and one.points.tolist() == [r.total_points]
    sq = sum((int(h) << 32) + int(lo) for h, lo in zip(r.sq_hi, r.sq_lo))
    n = r.total_in_points
    assert one.rmse_mm[0] == pytest.approx((sq / 4 / n) ** 0.5) and one.max_abs_mm[0] == r.max_abs_r2_all / 2
    assert one.bias_mm[0] == pytest.approx(r.total_sum_r2 / 2 / n) and one.mean_abs_mm[0] == pytest.approx(r.total_sum_abs_r2 / 2 / n)
    assert one.inlier_share[0] + one.above_share[0] + one.below_share[0] == pytest.approx(1.0)
    assert one.plane_share[0] == pytest.approx(r.total_plane_points / r.total_points)
    assert one.plane_in_share[0] == pytest.approx(r.total_plane_in / max(r.total_plane_points, 1))
    assert r.clip2 == cases.CLIP2 and one.max_abs_mm[0] <= cases.CLIP2 / 2
