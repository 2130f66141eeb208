"""The plane fit without a GPU: the numpy restatement tests/fit_ref against a brute force over Python integers and
against LAPACK, bs_plane_fit_apply through the library (host only, no context), the ABI surface, and the scene the
stage exists for on the CPU oracle."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "fit_ref"))
import cases as fc  # noqa: E402
import fit_ref as fr  # noqa: E402

NEW = ["bs_plane_fit", "bs_plane_fit_apply", "bs_plane_fit_dev", "bs_plane_fits_free"]


def small_case(seed):
    """a few dozen to a few hundred points on 1 .. 12 planes; some planes empty, tiny, degenerate or too large"""
    rng = np.random.default_rng(900 + seed)
    n, m = int(rng.integers(1, 400)), int(rng.integers(1, 13))
    xyz, plane = fc.patches(rng, n, m, spread=int(rng.choice([0, 2, 300, 50_000])), noise=int(rng.choice([0, 3])), junk=0.15)
    if seed % 6 == 0 and m > 1:
        plane[plane == 2] = 1  # plane 2 has no point
    if seed % 8 == 1:
        xyz[plane == 1, 2] = xyz[plane == 1, 0]  # plane 1 lies in x == z ...
        xyz[plane == 1, 1] = 7                   # ... on one line
    return xyz, plane, m


@pytest.mark.parametrize("seed", range(50))
def test_restatement_equals_the_brute_force(oracle, seed):
    xyz, plane, m = small_case(seed)
    f, b = fr.plane_fit(xyz, plane, m), fr.brute(xyz, plane, m)
    for k in fr.ARRAYS:
        got, want = getattr(f, k), np.array(b[k], fr.DTYPES[k]).reshape(getattr(f, k).shape)
        assert got.dtype == fr.DTYPES[k]
        assert np.array_equal(got.view(np.int64) if k == "normal" else got, want.view(np.int64) if k == "normal" else want), k
    assert np.array_equal(f.residual, np.array(b["residual"], np.int64).astype(np.int32))
    assert (f.status[f.n_points < 3] == 1).all() and set(np.unique(f.status)) <= {0, 1}


def test_verdict_boundary_in_the_restatement(oracle):
    """3 n D^2 against 2^63 with D = 2^23 - 1 (centroid 0): 2^63 / (3 D^2) = 43 690.68, so 43 690 points are fitted
    and the next even count, 43 692, is refused"""
    D = fc.LIM
    assert 3 * 43690 * D * D < 2 ** 63 <= 3 * 43691 * D * D
    for n, st in ((43690, 0), (43692, 2)):
        xyz = np.zeros((n, 3), np.int32)
        xyz[:, 0] = np.where(np.arange(n) % 2 == 0, D, -D)
        xyz[:, 1] = np.arange(n) % 5
        f = fr.plane_fit(xyz, np.ones(n, np.int32), 1)
        assert f.status[0] == st and f.center[0, 0] == 0 == f.center[0, 2] and f.n_points[0] == n
        assert (f.moment[0, 0] == n * D * D) == (st == 0) and (f.residual[0] == fr.I32_MIN) == (st == 2)


def test_normal_agrees_with_lapack(oracle):
    """|sin| of the angle to np.linalg.eigh's smallest eigenvector <= 1e-9 where the two smallest eigenvalues differ
    by more than 1 %"""
    checked = 0
    for seed in range(60):
        rng = np.random.default_rng(300 + seed)
        xyz, plane = fc.patches(rng, 3000, 6, spread=int(rng.choice([50, 2000, 60_000])), noise=int(rng.choice([1, 5, 200])),
                                junk=0.0)
        f = fr.plane_fit(xyz, plane, 6)
        for p in np.nonzero(f.status == 0)[0]:
            d = xyz[plane == p + 1].astype(np.float64) - xyz[plane == p + 1].astype(np.float64).mean(0)
            w, v = np.linalg.eigh(d.T @ d / len(d))
            if w[1] - w[0] <= 0.01 * w[1]:
                continue
            assert np.linalg.norm(np.cross(f.normal[p], v[:, 0])) <= 1e-9, (seed, p)
            assert f.normal[p, 2] >= 0 and abs(np.linalg.norm(f.normal[p]) - 1) < 1e-12
            checked += 1
    assert checked > 300


def test_apply_through_the_library_without_a_context():
    from buildingsegment_amd import _lib, api
    rng = np.random.default_rng(5)
    for m in (0, 1, 7, 300):
        status = rng.integers(0, 3, m).astype(np.int32)
        fit = api.PlaneFits(m, status, None, rng.integers(-9000, 9000, (m, 3)).astype(np.int32), rng.normal(size=(m, 3)),
                            None, None, None, None, None, None)
        normal, center = rng.normal(size=(m, 3)), rng.integers(-9000, 9000, (m, 3)).astype(np.int32)
        keep = normal.copy(), center.copy()
        nrm, ctr = api.plane_fit_apply(fit, normal, center)
        assert nrm.dtype == np.float64 and ctr.dtype == np.int32
        assert np.array_equal(nrm, np.where((status == 0)[:, None], fit.normal, normal))
        assert np.array_equal(ctr, np.where((status == 0)[:, None], fit.center, center))
        assert np.array_equal(normal, keep[0]) and np.array_equal(center, keep[1])  # new tables: the inputs stay
        want = fr.apply(fit, normal, center)
        assert np.array_equal(nrm, want[0]) and np.array_equal(ctr, want[1])
    L = _lib.load()
    st = _lib.PlaneFits()
    assert L.bs_plane_fit_apply(None, None, None) == -1 and L.bs_plane_fit_apply(C.byref(st), None, None) == 0
    st.n_planes = 2
    assert L.bs_plane_fit_apply(C.byref(st), None, None) == -1  # null arrays with planes
    st.n_planes = -1
    assert L.bs_plane_fit_apply(C.byref(st), None, None) == -1
    L.bs_plane_fits_free(C.byref(_lib.PlaneFits()))  # a zeroed struct
    L.bs_plane_fits_free(None)


def test_header_and_loader_name_the_new_functions():
    from buildingsegment_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bs_api.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bs_plane_fit[a-z_]*)\s*\(", txt))
    assert declared == set(NEW) == {s for s in _lib.EXPORTS if s.startswith("bs_plane_fit")}
    assert "#define BS_API_VERSION 5" in txt and "struct bs_plane_fits {" in txt
    L = _lib.load()
    assert all(hasattr(L, s) for s in NEW)
    fields = [k for k, _ in _lib.PlaneFits._fields_]
    body = txt[txt.index("struct bs_plane_fits {"):]
    body = body[:body.index("};")]
    assert fields == re.findall(r"\b(\w+);", body)  # the same members in the same order


def test_the_scene_the_stage_exists_for(oracle):
    """A tilted sheet far from the origin: segment()'s centre is the reference's wrapped 32-bit sum, the refitted plane
    is the sheet."""
    xyz = fc.tilted_sheet()
    neigh, normals = oracle.knn_normals(xyz, k=15)
    plane_idx, planes = oracle.region_grow(xyz, normals, neigh)
    n_planes = len(planes["id"])
    big = int(np.argmax(np.diff(planes["offset"])))
    own = xyz[plane_idx == big + 1].astype(np.int64)
    assert len(own) > 10_000
    # the quirk this feature exists for: x sums to more than 2^31 and the reference's int sum wraps
    assert own[:, 0].sum() > 2 ** 31 and abs(int(planes["center"][big][0]) - own[:, 0].mean()) > 1e6
    f = fr.plane_fit(xyz, plane_idx, n_planes)
    assert f.status[big] == 0 and f.n_points[big] == len(own)
    assert np.abs(f.center[big] - own.mean(0)).max() < 1 and f.r_abs_max[big] <= 12
    want = fc.sheet_z(own[:, 0], own[:, 1])
    H = np.trunc(fr.height_of(f.normal[big], f.center[big], own[:, 0], own[:, 1]))
    err = np.abs(H - want).max()
    print("refitted height error at the plane's own points:", err, "mm")
    assert err <= 5.0  # measured: 1.0 mm (0.47 mm before the truncation to an integer)
    H0 = fr.height_of(planes["normal"][big], planes["center"][big], own[:, 0], own[:, 1])
    assert np.abs(H0 - want).max() > 1e6  # segment()'s tables, unclamped: today's behaviour
