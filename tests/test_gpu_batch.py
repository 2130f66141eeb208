"""bs_segment_batch: n_tiles independent clouds in one device pass.  Every tile's output must equal what the
single-cloud path (and the CPU oracle) gives for that tile alone, bit for bit: neighbour rows (tile-local), normals,
labels (planes numbered from 1 per tile) and plane lists."""
import os

import numpy as np
import pytest

from buildingsegment_amd import api, synth
from buildingsegment_amd._lib import BsError

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))["xyz"]


def _planes_equal(a, b):
    assert len(a) == len(b), f"{len(a)} planes against {len(b)}"
    for x, y in zip(a, b):
        assert x.id == y.id
        assert np.array_equal(x.pointIdx, y.pointIdx)
        assert np.array_equal(x.center, y.center)
        assert np.array_equal(x.normal, y.normal)


def _same(res, want, what=""):
    neigh, normals, pi, planes = res
    wn, wr, wp, wpl = want
    assert np.array_equal(neigh, wn), f"{what}: {(neigh != wn).any(axis=1).sum()} rows differ"
    assert np.array_equal(normals, wr), f"{what}: normals differ"
    assert np.array_equal(pi, wp), f"{what}: {(pi != wp).sum()} labels differ"
    _planes_equal(planes, wpl)


def _oracle(O, xyz, p):
    ng, nr = O.knn_normals(xyz, k=p.k, radius=p.radius, max_nn=p.max_nn)
    pi, pl = O.region_grow(xyz, nr, ng, th_thickness=p.th_thickness, th_point_count=p.th_point_count, cos_th=p.cos_th)
    planes = [api.Plane(int(pl["id"][i]), pl["normal"][i], pl["center"][i],
                        pl["point_idx"][pl["offset"][i]:pl["offset"][i + 1]]) for i in range(len(pl["id"]))]
    return ng, nr, pi, planes


def _mixed():
    return [synth.plane_cube(), synth.facade(n_side=200, seed=4), synth.boxes(), synth.uniform(30000),
            _gold("walls_6k"), _gold("orphans_p5"), _gold("grid_patch_p1")]


_ORACLE = {}


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("k", (15, 16, 32))
def test_mixed_batch_matches_oracle_per_tile(gpu_ctx, oracle, k, mode):
    tiles = _mixed()
    p = api.default_params(k=k, rg_mode=mode)
    if k not in _ORACLE:
        _ORACLE[k] = [_oracle(oracle, x, p) for x in tiles]
    out = gpu_ctx.segment_batch(tiles, p)
    assert len(out) == len(tiles)
    for t, (res, want) in enumerate(zip(out, _ORACLE[k])):
        _same(res, want, f"tile {t}")
    assert sum(len(r[3]) for r in out) > 5  # (the batch does grow planes)


def test_repeated_cloud_gives_identical_results(gpu_ctx):
    x = synth.facade(n_side=150, seed=5)
    p = api.default_params(k=16)
    solo = gpu_ctx.segment(x, p)
    out = gpu_ctx.segment_batch([x] * 8, p)
    assert len(solo[3]) > 0
    for t, res in enumerate(out):
        _same(res, solo, f"copy {t}")


def test_touching_tiles_are_isolated(gpu_ctx):
    a = synth.plane_cube()[:40000].copy()
    b = a.copy()
    b[:, 0] += int(a[:, 0].max() - a[:, 0].min()) + 1  # the copy starts 1 mm past the first one's x extent
    p = api.default_params(k=15)
    out = gpu_ctx.segment_batch([a, b], p)
    _same(out[0], gpu_ctx.segment(a, p), "tile 0")
    _same(out[1], gpu_ctx.segment(b, p), "tile 1")
    # as ONE cloud the two copies do see each other: the isolation above is not vacuous
    merged = gpu_ctx.segment(np.concatenate([a, b]), p)[0]
    n = len(a)
    cross = (merged[:n] >= n).any(axis=1).sum() + (merged[n:] < n).any(axis=1).sum()
    assert cross > 0


def test_overlapping_tiles_are_isolated(gpu_ctx):
    c = synth.plane_cube()[:30000].copy()
    tiles = [synth.uniform(20000, seed=1), synth.uniform(20000, seed=2), c, c + 7]
    p = api.default_params(k=15)
    for t, res in enumerate(gpu_ctx.segment_batch(tiles, p)):
        _same(res, gpu_ctx.segment(tiles[t], p), f"tile {t}")


def test_batch_of_one_equals_segment(gpu_ctx):
    x = synth.plane_cube()
    for mode in (1, 2):
        p = api.default_params(k=15, rg_mode=mode)
        (res,) = gpu_ctx.segment_batch([x], p)
        _same(res, gpu_ctx.segment(x, p), f"rg_mode {mode}")


def _tiny_tiles(n_tiles=2000, seed=7, k=15):
    rng = np.random.default_rng(seed)
    tiles = []
    for t in range(n_tiles):
        m = k if t % 97 == 0 else int(rng.integers(15, 501))
        if t % 3 == 0:  # a noisy wall patch: planes grow in some tiles
            u = rng.integers(0, 3000, size=(m, 2))
            x = np.stack([u[:, 0], rng.integers(0, 20, size=m), u[:, 1]], axis=1)
        else:
            x = rng.integers(0, 1500, size=(m, 3))
        if t % 10 == 5 and m > 20:  # sparse outliers far outside every ring: the full-scan fallback of the tile
            x[:3] = rng.integers(3_000_000, 3_100_000, size=(3, 3))
        tiles.append(x.astype(np.int32))
    return tiles


def test_many_tiny_tiles(gpu_ctx, oracle):
    tiles = _tiny_tiles()
    p = api.default_params(k=15, th_point_count=100)
    want = [_oracle(oracle, x, p) for x in tiles]
    for mode in (1, 2):
        p.rg_mode = mode
        out = gpu_ctx.segment_batch(tiles, p)
        assert gpu_ctx.timings()["n_fallback_queries"] > 0
        for t in range(len(tiles)):
            _same(out[t], want[t], f"tile {t} (rg_mode {mode})")
    assert any(len(r[3]) for r in out)


def test_errors_leave_the_context_usable(gpu_ctx):
    x = synth.uniform(2000)
    p = api.default_params(k=15)
    with pytest.raises(BsError) as e:
        gpu_ctx.segment_batch([x, x[:10], x], p)
    assert e.value.status == -1 and "tile 1" in str(e.value)
    import torch
    d_xyz = torch.from_numpy(np.concatenate([x, x])).cuda()
    d_pi = torch.empty(2 * len(x), dtype=torch.int32, device="cuda")
    for bad in ([0, 3000, 2000, 4000], [5, 2000, 4000], [0, 2000, 1 << 31]):
        with pytest.raises(BsError) as e:
            gpu_ctx.segment_batch_dev(d_xyz.data_ptr(), bad, d_pi.data_ptr(), p)
        assert e.value.status == -1
    off = np.array([0], dtype=np.int64)
    assert gpu_ctx._L.bs_segment_batch_dev(gpu_ctx._h, d_xyz.data_ptr(), off.ctypes.data, 0, api.C.byref(p), None,
                                           None, d_pi.data_ptr()) == -1
    far = x.copy()
    far[17, 1] = 1 << 23
    with pytest.raises(BsError) as e:
        gpu_ctx.segment_batch([x, far], p)
    assert e.value.status == -2 and "tile 1" in str(e.value)
    out = gpu_ctx.segment_batch([x, x + 1], p)
    _same(out[0], gpu_ctx.segment(x, p))


def test_device_form_equals_host_form(gpu_ctx):
    import torch
    tiles = [synth.boxes(), synth.facade(n_side=120, seed=9), _gold("walls_6k")]
    p = api.default_params(k=16)
    host = gpu_ctx.segment_batch(tiles, p)
    xyz, off = api.pack_tiles(tiles)
    n = len(xyz)
    d_xyz = torch.from_numpy(xyz).cuda()
    d_neigh = torch.empty((n, p.k), dtype=torch.int32, device="cuda")
    d_nrm = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    d_pi = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu_ctx.segment_batch_dev(d_xyz.data_ptr(), off, d_pi.data_ptr(), p, d_neigh.data_ptr(), d_nrm.data_ptr())
    planes = gpu_ctx.batch_planes_fetch()
    neigh, nrm, pi = d_neigh.cpu().numpy(), d_nrm.cpu().numpy(), d_pi.cpu().numpy()
    for t in range(len(tiles)):
        s = slice(off[t], off[t + 1])
        _same((neigh[s], nrm[s], pi[s], planes[t]), host[t], f"tile {t}")


def test_audit_on_a_batch(gpu_ctx):
    tiles = [synth.plane_cube(), synth.boxes(), synth.facade(n_side=200, seed=4)]
    gpu_ctx.set_audit(True)
    try:
        gpu_ctx.segment_batch(tiles, api.default_params(k=15, rg_mode=2))
        tm = gpu_ctx.timings()
    finally:
        gpu_ctx.set_audit(False)
    assert tm["audit_mismatches"] == 0 and tm["audit_attempts"] == tm["n_seed_attempts"] > 0


def test_shift_tiles_to_origin(gpu_ctx):
    import torch
    raw = [synth.plane_cube()[:5000].astype(np.int64) + np.array([5_000_000, -3_000_000, 100_000]),
           synth.boxes()[:7000].astype(np.int64) - np.array([2_000_000, 0, 40_000]),
           synth.uniform(3000).astype(np.int64) + 123]
    tiles = [r.astype(np.int32) for r in raw]
    xyz, off = api.pack_tiles(tiles)
    d_xyz = torch.from_numpy(xyz).cuda()
    mn = gpu_ctx.shift_tiles_to_origin_dev(d_xyz.data_ptr(), off)
    got = d_xyz.cpu().numpy()
    for t, x in enumerate(tiles):
        d_one = torch.from_numpy(x.copy()).cuda()
        assert mn[t].tolist() == gpu_ctx.shift_to_origin_dev(d_one.data_ptr(), len(x)).tolist()
        assert np.array_equal(got[off[t]:off[t + 1]], d_one.cpu().numpy())
    # the host form's shift_to_origin gives each tile its solo result on the shifted tile
    p = api.default_params(k=15)
    out = gpu_ctx.segment_batch(tiles, p, shift_to_origin=True)
    for t, x in enumerate(tiles):
        _same(out[t], gpu_ctx.segment(got[off[t]:off[t + 1]], p), f"tile {t}")


def _solo_dev(ctx, d_xyz, n, p):
    import torch
    d_neigh = torch.empty((n, p.k), dtype=torch.int32, device="cuda")
    d_nrm = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    d_pi = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.segment_dev(d_xyz.data_ptr(), n, d_pi.data_ptr(), p, d_neigh.data_ptr(), d_nrm.data_ptr())
    return d_neigh, d_nrm, d_pi, ctx.planes_fetch()


@pytest.mark.parametrize("case", ["urban_16x250k", "facade_4x1m"])
def test_solo_equality_at_size(gpu_ctx, case):
    import torch
    if case == "urban_16x250k":
        tiles = [synth.urban(250_000, seed=100 + s) for s in range(16)]
    else:
        tiles = [synth.facade(n_side=1000, seed=2 + s) for s in range(4)]
    p = api.default_params(k=16)
    xyz, off = api.pack_tiles(tiles)
    n = len(xyz)
    d_xyz = torch.from_numpy(xyz).cuda()
    d_neigh = torch.empty((n, p.k), dtype=torch.int32, device="cuda")
    d_nrm = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    d_pi = torch.empty(n, dtype=torch.int32, device="cuda")
    gpu_ctx.segment_batch_dev(d_xyz.data_ptr(), off, d_pi.data_ptr(), p, d_neigh.data_ptr(), d_nrm.data_ptr())
    planes = gpu_ctx.batch_planes_fetch()
    for t in range(len(tiles)):
        s = slice(int(off[t]), int(off[t + 1]))
        sn, sr, sp, spl = _solo_dev(gpu_ctx, d_xyz[s].contiguous(), int(off[t + 1] - off[t]), p)
        assert torch.equal(d_neigh[s], sn), f"tile {t}: rows differ"
        assert torch.equal(d_nrm[s], sr), f"tile {t}: normals differ"
        assert torch.equal(d_pi[s], sp), f"tile {t}: labels differ"
        _planes_equal(planes[t], spl)
