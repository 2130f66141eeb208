"""bs_grid_picture_batch[_dev] and bs_tile_boxes_dev: every tile's raster and ground threshold must equal, bit for
bit, what bs_grid_picture returns for that tile alone (and the reference's golden images / the CPU oracle)."""
import glob
import os

import numpy as np
import pytest

from buildingsegment_amd import api, synth
from buildingsegment_amd._lib import BsError

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "raster_*.npz")))
pytestmark = pytest.mark.gpu


def _urban_tiles(n_tiles, n, seed=0):
    return [synth.shift_to_origin(synth.urban(n, seed=seed + t)) for t in range(n_tiles)]


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch has no device")
    return torch


def test_golden_fixtures_as_one_batch(gpu_ctx, oracle):
    gs = [np.load(p) for p in FIXTURES]
    tiles = [(g["xyz"] - g["box_min"]).astype(np.int32) for g in gs]
    exts = np.array([(g["box_max"] - g["box_min"]) for g in gs], dtype=np.int32)
    res = gpu_ctx.grid_picture_batch(tiles, extents=exts)
    assert len(res) == len(gs)
    for g, sh, ext, (img, th) in zip(gs, tiles, exts, res):
        assert img.shape == (int(g["height"]), int(g["width"]), 3)
        assert th == float(g["ground_th"])
        assert np.array_equal(img[..., 0], g["image"][..., 0])
        assert np.array_equal(img[..., 2], g["image"][..., 2])
        ref1 = g["image"][..., 1]
        assert (np.abs(img[..., 1] - ref1) <= np.spacing(np.abs(ref1))).all()
        simg, sth = gpu_ctx.grid_picture(sh, extent=ext)
        oimg, oth = oracle.grid_picture(sh, extent=ext)
        assert sth == th == oth and np.array_equal(img, simg) and np.array_equal(img, oimg)


@pytest.mark.parametrize("bin_,bh", [(100, 1000), (37, 250)])
def test_urban_tiles_equal_solo(gpu_ctx, oracle, bin_, bh):
    rng = np.random.default_rng(bin_)
    tiles = _urban_tiles(6, 60_000, seed=5)
    tiles.append(rng.integers(0, 4000, (30_000, 3)).astype(np.int32))       # uniform block
    tiles.append(np.array([[0, 0, 0]], np.int32))                            # a single point
    tiles.append(synth.shift_to_origin(synth.urban(150_000, seed=99)))       # a larger one
    res = gpu_ctx.grid_picture_batch(tiles, bin=bin_, bin_height=bh)
    for t, (img, th) in enumerate(res):
        simg, sth = gpu_ctx.grid_picture(tiles[t], bin=bin_, bin_height=bh)
        assert th == sth, f"tile {t}"
        assert np.array_equal(img, simg), f"tile {t}: {(img != simg).any(-1).sum()} pixels differ"
        oimg, oth = oracle.grid_picture(tiles[t], bin=bin_, bin_height=bh)  # the solo call is a batch of one
        assert th == oth and np.array_equal(img, oimg), f"tile {t} against the oracle"


def test_point_order_is_respected_per_tile(gpu_ctx, oracle):
    rng = np.random.default_rng(3)
    xyz = rng.integers(0, 3000, (200_000, 3)).astype(np.int32)
    xyz[0] = 0
    xyz[1] = 2999
    perm = rng.permutation(len(xyz))
    other = _urban_tiles(1, 50_000, seed=7)[0]
    res = gpu_ctx.grid_picture_batch([other, xyz, xyz[perm], other])
    oa, _ = oracle.grid_picture(xyz)
    ob, _ = oracle.grid_picture(xyz[perm])
    assert not np.array_equal(oa, ob)  # the order matters
    assert np.array_equal(res[1][0], oa) and np.array_equal(res[2][0], ob)
    assert np.array_equal(res[0][0], res[3][0])


def test_shift_to_origin_option(gpu_ctx, oracle):
    rng = np.random.default_rng(4)
    raw = [rng.integers(-50_000, 90_000, (20_000, 3)).astype(np.int32) + rng.integers(0, 10 ** 6, 3).astype(np.int32)
           for _ in range(4)]
    res = gpu_ctx.grid_picture_batch(raw, shift_to_origin=True)
    for t in range(4):
        simg, sth = gpu_ctx.grid_picture(synth.shift_to_origin(raw[t]))
        assert res[t][1] == sth and np.array_equal(res[t][0], simg)
        oimg, oth = oracle.grid_picture(synth.shift_to_origin(raw[t]))
        assert res[t][1] == oth and np.array_equal(res[t][0], oimg)


def test_device_form_and_tile_boxes(gpu_ctx):
    torch = _torch()
    rng = np.random.default_rng(5)
    raw = [synth.urban(40_000, seed=20 + t) + rng.integers(-10 ** 6, 10 ** 6, 3).astype(np.int32) for t in range(5)]
    xyz, off = api.pack_tiles(raw)
    d = torch.from_numpy(xyz).cuda()
    box = gpu_ctx.tile_boxes_dev(d.data_ptr(), off)
    for t in range(5):
        part = xyz[off[t]:off[t + 1]]
        assert np.array_equal(box[t], np.concatenate([part.min(0), part.max(0)]))
    mn = gpu_ctx.shift_tiles_to_origin_dev(d.data_ptr(), off)
    assert np.array_equal(mn, box[:, :3])
    box2 = gpu_ctx.tile_boxes_dev(d.data_ptr(), off)
    ext = box2[:, 3:] - box2[:, :3]
    assert (box2[:, :3] == 0).all()
    w, h, po = api.grid_dims_batch(ext)
    img = torch.empty(3 * int(po[-1]), dtype=torch.float64, device="cuda")
    th = gpu_ctx.grid_picture_batch_dev(d.data_ptr(), off, ext, img.data_ptr())
    host = gpu_ctx.grid_picture_batch([synth.shift_to_origin(r) for r in raw], extents=ext)
    himg = img.cpu().numpy()
    for t in range(5):
        assert th[t] == host[t][1]
        assert np.array_equal(himg[3 * po[t]:3 * po[t + 1]].reshape(h[t], w[t], 3), host[t][0])


def test_point_outside_its_extent_names_the_tile(gpu_ctx):
    tiles = _urban_tiles(5, 20_000, seed=40)
    exts = np.array([t.max(0) for t in tiles], np.int32)
    for bad in (3, 1):
        e = exts.copy()
        e[bad, 0] -= 1  # the tile's own max x now lies outside
        with pytest.raises(BsError) as ei:
            gpu_ctx.grid_picture_batch(tiles, extents=e)
        assert ei.value.status == -2 and f"tile {bad}" in str(ei.value)
    e = exts.copy()
    e[4, 2] -= 1
    e[2, 1] -= 1
    with pytest.raises(BsError) as ei:
        gpu_ctx.grid_picture_batch(tiles, extents=e)
    assert ei.value.status == -2 and "tile 2" in str(ei.value)  # the smallest failing tile
    # the context still works
    img, th = gpu_ctx.grid_picture_batch(tiles, extents=exts)[4]
    simg, sth = gpu_ctx.grid_picture(tiles[4], extent=exts[4])
    assert th == sth and np.array_equal(img, simg)


def test_malformed_offsets_and_parameters(gpu_ctx):
    L, h = gpu_ctx._L, gpu_ctx._h
    xyz = np.zeros((10, 3), np.int32)
    ext = np.zeros((3, 3), np.int32)
    img = np.zeros(3 * 100, np.float64)

    def call(off, n_tiles, e=ext, bin_=100, bh=1000):
        off = np.ascontiguousarray(off, dtype=np.int64)
        return L.bs_grid_picture_batch(h, xyz.ctypes.data, off.ctypes.data, n_tiles, e.ctypes.data, bin_, bh,
                                       img.ctypes.data, None)

    for off, nt in (([1, 4, 10], 2), ([0, 4, 4, 10], 3), ([0, 6, 4, 10], 3), ([0, 10], 0)):
        assert call(off, nt) == -1, off
    msg = L.bs_last_error(h).decode()
    assert "n_tiles" in msg
    assert call([0, 4, 4, 10], 3) == -1 and "tile 1" in L.bs_last_error(h).decode()
    bad = ext.copy()
    bad[2, 2] = -1
    assert call([0, 3, 6, 10], 3, e=bad) == -1 and "tile 2" in L.bs_last_error(h).decode()
    assert call([0, 3, 6, 10], 3, bin_=0) == -1
    assert call([0, 3, 6, 10], 3, bh=0) == -1
    assert call([0, 3, 6, 10], 3) == 0  # the context still works


def test_many_small_tiles(gpu_ctx, oracle):
    rng = np.random.default_rng(8)
    tiles = [rng.integers(0, rng.integers(1, 3000), (int(rng.integers(1, 400)), 3)).astype(np.int32)
             for _ in range(2000)]
    res = gpu_ctx.grid_picture_batch(tiles, shift_to_origin=True)
    for t in range(0, 2000, 97):
        simg, sth = gpu_ctx.grid_picture(synth.shift_to_origin(tiles[t]))
        assert res[t][1] == sth and np.array_equal(res[t][0], simg), f"tile {t}"
    for t in range(0, 2000, 50):
        oimg, oth = oracle.grid_picture(synth.shift_to_origin(tiles[t]))
        assert res[t][1] == oth and np.array_equal(res[t][0], oimg), f"tile {t} against the oracle"
