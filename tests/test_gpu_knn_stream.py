"""Stages 1-2 three ways: the default build (ring 1 of knn_fast2_kernel as one candidate stream per lane, the accepted
trial binning reused as the grid's sort), BS_KNN_STREAM=0 (the loop per cell) and BS_GRID_REUSE=0 (step 3 of build_grid
always sorts again).  Both switches are read in every call.  Neighbour rows, the 64-bit patterns of the normals,
tie_rows and fallback_queries must be equal bit for bit between the three, and equal to the CPU oracle where the cloud
has at most 20 k points."""
import os

import numpy as np
import pytest

from buildingsegment_amd import api

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
MODES = ((), (("BS_KNN_STREAM", "0"),), (("BS_GRID_REUSE", "0"),))


def _gold(name):
    return np.ascontiguousarray(np.load(os.path.join(GOLD, name + ".npz"))["xyz"], dtype=np.int32)


def _set(monkeypatch, mode):
    for name in ("BS_KNN_STREAM", "BS_GRID_REUSE"):
        monkeypatch.delenv(name, raising=False)
    for name, value in mode:
        monkeypatch.setenv(name, value)


def _three_ways(ctx, O, monkeypatch, xyz, k, **kw):
    """-> (neigh, normals, tie_rows, fallback_queries) of the default run, after the comparisons"""
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    p = api.default_params(k=k, **kw)
    runs = []
    for mode in MODES:
        _set(monkeypatch, mode)
        neigh, normals = ctx.knn_normals(xyz, p)
        tm = ctx.timings()
        runs.append((neigh, normals, tm["tie_rows"], tm["n_fallback_queries"]))
    _set(monkeypatch, ())
    ref = runs[0]
    for mode, run in zip(MODES[1:], runs[1:]):
        assert np.array_equal(run[0], ref[0]), f"{mode}: {(run[0] != ref[0]).any(axis=1).sum()} rows differ"
        assert np.array_equal(run[1].view(np.int64), ref[1].view(np.int64)), f"{mode}: normals differ"
        assert run[2] == ref[2], f"{mode}: tie_rows {run[2]} against {ref[2]}"
        assert run[3] == ref[3], f"{mode}: fallback_queries {run[3]} against {ref[3]}"
    if len(xyz) <= 20000:
        oneigh, onormals = O.knn_normals(xyz, k=k, radius=p.radius, max_nn=p.max_nn)
        assert np.array_equal(ref[0], oneigh), f"{(ref[0] != oneigh).any(axis=1).sum()} rows differ from the oracle"
        assert np.array_equal(ref[1].view(np.int64), onormals.view(np.int64)), "normals differ from the oracle"
    return ref


def _sheet(nx, ny, spacing, z=0):
    u, v = np.meshgrid(np.arange(nx) * spacing, np.arange(ny) * spacing, indexing="ij")
    return np.stack([u.ravel(), v.ravel(), np.full(u.size, z)], 1).astype(np.int32)


def _sheet_and_clump():
    """5 003 points: a 50 mm sheet and 700 points inside one 20 mm cube above its middle (one cell at the 132 mm edge the
    rule chooses: a range far longer than a batch next to lanes with nearly empty streams), in a fixed shuffle."""
    rng = np.random.default_rng(31)
    sheet = _sheet(67, 65, 50)[:4303]
    clump = rng.integers(0, 20, (700, 3)) + np.array([1600, 1600, 20])
    xyz = np.concatenate([sheet, clump]).astype(np.int32)
    assert len(xyz) == 5003
    return xyz[rng.permutation(len(xyz))]


@pytest.mark.parametrize("name,k", [("facade_10k_k16", 16), ("facade_10k_k16", 15), ("plane_cube_12k", 16),
                                    ("plane_cube_12k", 15), ("walls_6k", 32)])
def test_golden_clouds(gpu_ctx, oracle, monkeypatch, name, k):
    """k = 15 is K < KC (the runner-up is the list's slot K), k = 32 the <32> instances."""
    _three_ways(gpu_ctx, oracle, monkeypatch, _gold(name), k)


@pytest.mark.parametrize("radius", [181.0, 182.0, 250.0])
def test_radius_around_the_moment_switch(gpu_ctx, oracle, monkeypatch, radius):
    """r <= 181 mm keeps the moment sums relative in 32 bits, above it the 64-bit instance runs."""
    _three_ways(gpu_ctx, oracle, monkeypatch, _gold("facade_10k_k16"), 16, radius=radius)


def test_lattice_ties_everywhere(gpu_ctx, oracle, monkeypatch):
    g = np.arange(24)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    ref = _three_ways(gpu_ctx, oracle, monkeypatch, lat * 40, 16)
    assert ref[2] > 0
    # 20 mm: a corner's r = 100 mm ball still holds more than max_nn = 50 points -- every query is work-listed
    ref = _three_ways(gpu_ctx, oracle, monkeypatch, lat * 20, 16)
    assert ref[3] == len(lat)


def test_uneven_streams_in_one_wave(gpu_ctx, oracle, monkeypatch):
    xyz = _sheet_and_clump()
    _three_ways(gpu_ctx, oracle, monkeypatch, xyz, 16)
    _three_ways(gpu_ctx, oracle, monkeypatch, xyz[:37], 16)  # one partial wave


def test_lanes_that_go_on_to_ring_2(gpu_ctx, oracle, monkeypatch):
    """A 50 mm sheet and 200 isolated points on a 400 mm lattice beside it: those are not certified after ring 1.  (The
    API does not return the cell edge: a k-th distance above 300 mm stands for "more than two cell edges".)"""
    g = np.arange(6)
    iso = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:200] * 400 + np.array([3600, 0, 400]))
    xyz = np.concatenate([_sheet(67, 65, 50), iso]).astype(np.int32)
    rng = np.random.default_rng(32)
    xyz = xyz[rng.permutation(len(xyz))]
    neigh = _three_ways(gpu_ctx, oracle, monkeypatch, xyz, 16)[0]
    d = xyz[neigh[:, -1]].astype(np.int64) - xyz
    assert (np.sqrt((d * d).sum(1)) > 300).any()


@pytest.mark.parametrize("mirror", [False, True])
def test_domain_edges(gpu_ctx, oracle, monkeypatch, mirror):
    xyz = _sheet_and_clump().astype(np.int64)
    xyz += (1 << 23) - 2 - xyz.max()
    assert xyz.max() == (1 << 23) - 2
    _three_ways(gpu_ctx, oracle, monkeypatch, -xyz if mirror else xyz, 16)


def test_batch_equals_solo_calls(gpu_ctx, monkeypatch):
    """Three tiles through bs_segment_batch (the tiled instances and build_grid_tiled), each run against the per-tile
    solo calls of the same run."""
    big = _gold("facade_10k_k16")[:9000]
    tiles = [np.ascontiguousarray(big[:3000]), _sheet_and_clump()[:40].copy(), big]
    assert [len(t) for t in tiles] == [3000, 40, 9000]
    p = api.default_params(k=16)
    first = None
    for mode in MODES:
        _set(monkeypatch, mode)
        out = gpu_ctx.segment_batch(tiles, p)
        tm = gpu_ctx.timings()
        for t, res in enumerate(out):
            solo = gpu_ctx.segment(tiles[t], p)
            assert np.array_equal(res[0], solo[0]), f"{mode} tile {t}: rows differ from the solo call"
            assert np.array_equal(res[1].view(np.int64), solo[1].view(np.int64)), f"{mode} tile {t}: normals differ"
            assert np.array_equal(res[2], solo[2]), f"{mode} tile {t}: labels differ"
        cur = (out, tm["tie_rows"], tm["n_fallback_queries"])
        if first is None:
            first = cur
        else:
            assert cur[1:] == first[1:], f"{mode}: tie_rows / fallback_queries {cur[1:]} against {first[1:]}"
            for a, b in zip(out, first[0]):
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
    _set(monkeypatch, ())


def _grid_trials(xyz, k, radius):
    """build_grid's cell-size rule on the CPU -> (trial binnings, cell edge)"""
    xyz = xyz.astype(np.int64)
    mn = xyz.min(0)
    ext = int((xyz.max(0) - mn).max()) + 1
    target = max(4.0, 0.5 * k)
    cell = cmin = max(1, int(np.ceil(radius)))
    trials = 0
    for _ in range(4):
        trials += 1
        occ = len(xyz) / len(np.unique((xyz - mn) // cell, axis=0))
        if 0.7 * target <= occ <= 1.6 * target:
            break
        f = min(4.0, max(0.25, np.sqrt(target / occ)))
        ncell = max(int(np.floor(cell * f + 0.5)), cmin)
        if ncell == cell or ncell > ext:
            break
        cell = ncell
    return trials, cell


@pytest.mark.parametrize("spacing,trials", [(20, 1), (50, 2), (200, 3)])
def test_trial_counts_of_the_grid(gpu_ctx, oracle, monkeypatch, spacing, trials):
    """Sheets that need one, two and three trial binnings (computed here with build_grid's rule: 20 mm leaves at trial 1
    with the cell at its minimum, 50 mm accepts 142 mm at trial 2, 200 mm accepts 563 mm at trial 3; the library does
    not report the count).  With one trial step 3 sorts as before; with two or three the accepted trial is the grid's
    sort.  The sorted order itself is not returned by the API: the rows, normals, labels and planes that are computed in
    that order must be identical with BS_GRID_REUSE=0."""
    xyz = _sheet(80, 75, spacing)
    rng = np.random.default_rng(34)
    xyz = xyz[rng.permutation(len(xyz))]
    got, cell = _grid_trials(xyz, 16, 100.0)
    assert got == trials if trials < 3 else got >= 3, (got, cell)
    _three_ways(gpu_ctx, oracle, monkeypatch, xyz, 16)
    p = api.default_params(k=16)
    ref = gpu_ctx.segment(xyz, p)
    monkeypatch.setenv("BS_GRID_REUSE", "0")
    res = gpu_ctx.segment(xyz, p)
    monkeypatch.delenv("BS_GRID_REUSE")
    assert np.array_equal(res[0], ref[0]) and np.array_equal(res[1].view(np.int64), ref[1].view(np.int64))
    assert np.array_equal(res[2], ref[2]) and len(res[3]) == len(ref[3])
    for a, b in zip(res[3], ref[3]):
        assert np.array_equal(a.pointIdx, b.pointIdx) and np.array_equal(a.normal, b.normal)
