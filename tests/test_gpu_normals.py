"""Every leaf of the eigen-solver through every way the kernels build the moment sums.

The clouds of tests/normal_ref/cases.py are isolated clusters: the hybrid neighbourhood of each point of a cluster of at
most max_nn points is the cluster, and which leaf of bs_normal.h it takes is known from the traced restatement
(tests/test_normals_cpu.py prints the table).  Every call below asserts
  - the neighbour rows equal the oracle's,
  - the normals equal the oracle's as 64-bit patterns,
  - all points of a cluster of at most max_nn points carry the same 64-bit patterns (needs no oracle: a moment path
    whose error depends on the query, such as REL32's conversion to absolute sums, breaks it),
  - the premise that puts the call on the intended kernel: n_fallback_queries, computed here from the cluster sizes.
The switches (BS_KNN_*) are read on every call."""
import os
import sys

import numpy as np
import pytest

from buildingsegment_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.join(HERE, "fit_ref")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from normal_ref import cases  # noqa: E402
import fit_ref as fr  # noqa: E402

pytestmark = pytest.mark.gpu

SWITCHES = ("BS_KNN_STREAM", "BS_KNN_MOMENTS64", "BS_KNN_BUFFERED", "BS_KNN_GENERAL_THREAD")
_ORACLE = {}


def _set(monkeypatch, **env):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _oracle(O, key, xyz, p):
    """the oracle's rows and normals, computed once per (cloud, k, radius, max_nn) and never written to"""
    key = (key, p.k, p.radius, p.max_nn)
    if key not in _ORACLE:
        neigh, normals = O.knn_normals(xyz, k=p.k, radius=p.radius, max_nn=p.max_nn)
        neigh.setflags(write=False)
        normals.setflags(write=False)
        _ORACLE[key] = (neigh, normals)
    return _ORACLE[key]


def _shared(normals, cid, sizes, max_nn, what):
    """all points of a cluster of at most max_nn points carry the same bits"""
    bits = normals.view(np.int64)
    first = np.full(len(sizes), -1)
    first[cid[::-1]] = np.arange(len(cid))[::-1]
    whole = sizes[cid] <= max_nn
    bad = whole & (bits != bits[first[cid]]).any(axis=1)
    assert not bad.any(), f"{what}: the points of clusters {np.unique(cid[bad])[:8]} do not share one normal"


def _check(ctx, O, key, xyz, cid, sizes, p, expect_fallback, what=""):
    neigh, normals = ctx.knn_normals(xyz, p)
    fb = ctx.timings()["n_fallback_queries"]
    oneigh, onormals = _oracle(O, key, xyz, p)
    assert np.array_equal(neigh, oneigh), f"{what}: {(neigh != oneigh).any(axis=1).sum()} rows differ from the oracle"
    diff = (normals.view(np.int64) != onormals.view(np.int64)).any(axis=1)
    assert not diff.any(), (f"{what}: {diff.sum()} normals differ from the oracle, first in clusters "
                            f"{np.unique(cid[diff])[:8] if cid is not None else np.nonzero(diff)[0][:8]}")
    if cid is not None:
        _shared(normals, cid, sizes, p.max_nn, what)
    assert fb == expect_fallback, f"{what}: n_fallback_queries {fb}, expected {expect_fallback}"
    return neigh, normals


def _params(**kw):
    kw.setdefault("k", 3)
    kw.setdefault("radius", cases.RADIUS)
    kw.setdefault("max_nn", 64)
    return api.default_params(**kw)


@pytest.mark.parametrize("where", ["near", "domain"])
def test_rel32_fast_path(gpu_ctx, oracle, monkeypatch, where):
    """r = 181 mm: knn_fast2_kernel<16, REL32>, ring 1 as streams and as the loop per cell; no query is work-listed"""
    xyz, cid, sizes = cases.committed_cloud(where)
    for env in ({}, {"BS_KNN_STREAM": "0"}):
        _set(monkeypatch, **env)
        _check(gpu_ctx, oracle, where, xyz, cid, sizes, _params(), 0, f"{where} {env}")


@pytest.mark.parametrize("where", ["near", "domain"])
def test_moments64_fast_path(gpu_ctx, oracle, monkeypatch, where):
    """the same clouds with absolute 64-bit moments (both ring-1 forms), and through the first fast kernel"""
    xyz, cid, sizes = cases.committed_cloud(where)
    for env in ({"BS_KNN_MOMENTS64": "1"}, {"BS_KNN_MOMENTS64": "1", "BS_KNN_STREAM": "0"}, {"BS_KNN_BUFFERED": "0"}):
        _set(monkeypatch, **env)
        _check(gpu_ctx, oracle, where, xyz, cid, sizes, _params(), 0, f"{where} {env}")


@pytest.mark.parametrize("where", ["near", "domain"])
def test_radius_above_the_rel32_limit(gpu_ctx, oracle, monkeypatch, where):
    """clusters, pitch and radius times three: r = 543 mm takes the 64-bit instance by itself"""
    _set(monkeypatch)
    xyz, cid, sizes = cases.committed_cloud(where, 3 * cases.PITCH, 3)
    _check(gpu_ctx, oracle, where + "*3", xyz, cid, sizes, _params(radius=3 * cases.RADIUS), 0, where)


def _wave_cloud():
    # 200 mm cells, clusters every four cells: the 16th neighbour of a point of a smaller cluster is at least 700 mm
    # away, beyond the 600 mm two rings certify at most; a cluster of 16 .. 50 points is certified after ring 1
    clusters, _ = cases.case_list()
    xyz, cid, sizes = cases.cloud(clusters, 800, "near", k=16)
    return xyz, cid, sizes, int(sizes[(sizes < 16) | (sizes > 50)].sum())


def test_wave_kernel_and_one_thread_kernel(gpu_ctx, oracle, monkeypatch):
    xyz, cid, sizes, listed = _wave_cloud()
    assert 0 < listed < len(xyz)
    p = _params(k=16, max_nn=50, cell_size=200)
    _set(monkeypatch)
    _check(gpu_ctx, oracle, "wave", xyz, cid, sizes, p, listed, "wave kernel")
    _set(monkeypatch, BS_KNN_GENERAL_THREAD="1")
    _check(gpu_ctx, oracle, "wave", xyz, cid, sizes, p, listed, "one-thread kernel")


def test_mark_all_above_the_fast_cell_limit(gpu_ctx, oracle, monkeypatch):
    """cell_size > 7 500: no fast kernel, mark_all_kernel lists every query"""
    _set(monkeypatch)
    clusters, _ = cases.case_list()
    sub = [c for c in clusters if c["family"] in ("collinear", "ident", "tri", "needle")]
    xyz, cid, sizes = cases.cloud(sub, cases.PITCH, "near")
    _check(gpu_ctx, oracle, "sub", xyz, cid, sizes, _params(cell_size=7501), len(xyz), "mark_all")


@pytest.mark.parametrize("cell", [7500, 7501])
def test_fast_cell_limit_far_corner(gpu_ctx, oracle, monkeypatch, cell):
    """The last cell edge the fast kernels take, and the first they do not, on a cloud whose third neighbours lie in the
    far corner of the 5 x 5 x 5 block (d^2 = 3 * 22 499^2).  Two rings certify neither the 3-list nor the radius: every
    query is work-listed either way."""
    _set(monkeypatch)
    xyz, radius = cases.corner_cloud(7500)
    p = _params(radius=radius, max_nn=50, cell_size=cell)
    _check(gpu_ctx, oracle, "corner", xyz, None, None, p, len(xyz), f"cell {cell}")


@pytest.mark.parametrize("max_nn", [3, 50, 64])
def test_max_nn_boundary(gpu_ctx, oracle, monkeypatch, max_nn):
    """clusters of max_nn - 1, max_nn, max_nn + 1 points: exactly the points of the oversize clusters are work-listed
    and keep their nearest max_nn by (d^2, index); the others share their cluster's normal"""
    xyz, cid, sizes, k = cases.boundary_cloud(max_nn)
    listed = int(sizes[sizes > max_nn].sum())
    assert listed == 6 * (max_nn + 1)
    for env in ({}, {"BS_KNN_MOMENTS64": "1"}, {"BS_KNN_GENERAL_THREAD": "1"}):
        _set(monkeypatch, **env)
        _check(gpu_ctx, oracle, ("boundary", max_nn), xyz, cid, sizes, _params(k=k, max_nn=max_nn), listed, f"{env}")


def test_tiled_instances_equal_the_solo_calls(gpu_ctx, oracle, monkeypatch):
    """bs_segment_batch: the REL32 tiled instance, and with 64-bit moments the <16, 64-bit, TILED> instance, which
    runs without STREAM.  (The domain cloud goes in as it is: it spans the whole admissible box already.)"""
    tiles = [cases.committed_cloud("near"), cases.committed_cloud("domain"), cases.boundary_cloud(64)[:3]]
    keys = ["near", "domain", ("boundary", 64)]
    p = _params()
    for env in ({}, {"BS_KNN_MOMENTS64": "1"}):
        _set(monkeypatch, **env)
        out = gpu_ctx.segment_batch([t[0] for t in tiles], p)
        listed = gpu_ctx.timings()["n_fallback_queries"]
        assert listed == 6 * 65, f"{env}: n_fallback_queries {listed}"
        for key, (xyz, cid, sizes), res in zip(keys, tiles, out):
            solo = gpu_ctx.knn_normals(xyz, p)
            assert np.array_equal(res[0], solo[0]), f"{env} tile {key}: rows differ from the solo call"
            assert np.array_equal(res[1].view(np.int64), solo[1].view(np.int64)), f"{env} tile {key}: normals differ"
            oneigh, onormals = _oracle(oracle, key, xyz, p)
            assert np.array_equal(res[0], oneigh), f"{env} tile {key}: rows differ from the oracle"
            assert np.array_equal(res[1].view(np.int64), onormals.view(np.int64)), f"{env} tile {key}: normals differ from the oracle"
            _shared(res[1], cid, sizes, p.max_nn, f"{env} tile {key}")


@pytest.mark.parametrize("where", ["near", "domain"])
def test_plane_fit_every_cluster_one_plane(gpu_ctx, oracle, where):
    """the solver's second caller: bs_fit.hip forms its covariance from the deviations from the integer centroid"""
    xyz, cid, sizes = cases.committed_cloud(where)
    lab = (cid + 1).astype(np.int32)
    got = gpu_ctx.plane_fit(xyz, lab, len(sizes))
    ref = fr.plane_fit(xyz, lab, len(sizes))
    assert (ref.status == 0).all() and np.array_equal(got.status, ref.status)
    assert np.array_equal(got.dev_sum, ref.dev_sum) and np.array_equal(got.moment, ref.moment)
    diff = (got.normal.view(np.int64) != ref.normal.view(np.int64)).any(axis=1)
    assert not diff.any(), f"the fitted normals of clusters {np.nonzero(diff)[0][:8]} differ from tests/fit_ref"


def test_halo_slabs(gpu_ctx, oracle, monkeypatch):
    """bs_knn_normals_halo on the 'near' cloud cut in two between cluster columns, each slab with the foreign points
    up to 600 mm beyond the cut as halo (one column of clusters); every 3-list is certified inside 300 mm"""
    _set(monkeypatch)
    xyz, cid, sizes = cases.committed_cloud("near")
    p = _params()
    oneigh, onormals = _oracle(oracle, "near", xyz, p)
    cut = 4 * cases.PITCH + cases.BOX + 200
    for own, halo in ((xyz[:, 0] < cut, (xyz[:, 0] >= cut) & (xyz[:, 0] < cut + 600)),
                      (xyz[:, 0] >= cut, (xyz[:, 0] < cut) & (xyz[:, 0] >= cut - 600))):
        own_idx, halo_idx = np.nonzero(own)[0].astype(np.int32), np.nonzero(halo)[0].astype(np.int32)
        assert len(own_idx) > 1000 and len(halo_idx) > 100
        gidx = np.concatenate([own_idx, halo_idx])
        neigh, normals, unc = gpu_ctx.knn_normals_halo(xyz[gidx], gidx, len(own_idx), p, 300.0)
        assert unc == 0
        assert np.array_equal(neigh, oneigh[own_idx]), "rows differ from the oracle"
        assert np.array_equal(normals.view(np.int64), onormals[own_idx].view(np.int64)), "normals differ from the oracle"
        _shared_own = np.unique(cid[own_idx], return_inverse=True)
        _shared(normals, _shared_own[1], sizes[_shared_own[0]], p.max_nn, "halo slab")
