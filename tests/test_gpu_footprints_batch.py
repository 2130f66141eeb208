"""bs_footprints_batch[_dev]: every tile's contours, their order, areas, perimeters, closed mask and OBJ bytes must
equal the solo bs_footprints result for that tile alone and the sequential restatement tests/footprint_ref."""
import glob
import os
import sys

import numpy as np
import pytest

from buildingsegment_amd import api, synth
from buildingsegment_amd._lib import BsError

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
import ref  # noqa: E402
from test_gpu_footprints import SHAPES  # noqa: E402  (rings, nested, checker, spiral, comb, blobs, edges)

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "raster_*.npz")))
pytestmark = pytest.mark.gpu


def _same(a, b, what):
    assert len(a.contours) == len(b.contours), f"{what}: {len(a.contours)} contours against {len(b.contours)}"
    for i, (x, y) in enumerate(zip(a.contours, b.contours)):
        assert np.array_equal(x, y), f"{what}: contour {i} differs"
    assert np.array_equal(a.area, b.area), what
    assert np.array_equal(a.perimeter, b.perimeter), what


def _check_batch(ctx, images, tmp_path=None, with_ref=True, **kw):
    fps, masks = ctx.footprints_batch(images, return_mask=True, **kw)
    assert len(fps) == len(masks) == len(images)
    for t, img in enumerate(images):
        fp, mask = fps[t], masks[t]
        assert (fp.width, fp.height) == (img.shape[1], img.shape[0])
        solo, smask = ctx.footprints(img, return_mask=True, **kw)
        _same(fp, solo, f"tile {t} against solo")
        assert np.array_equal(mask, smask), f"tile {t}: mask"
        if with_ref:
            r, rmask = ref.footprints(img, **kw)
            _same(fp, r, f"tile {t} against the restatement")
            assert np.array_equal(mask, rmask * 255)
        if tmp_path is not None:
            api.write_footprints_obj(fp, tmp_path / "batch.obj")
            api.write_footprints_obj(solo, tmp_path / "solo.obj")
            assert (tmp_path / "batch.obj").read_bytes() == (tmp_path / "solo.obj").read_bytes(), f"tile {t}: OBJ"
    return fps


def _golden_images(ctx):
    out = []
    for p in FIXTURES:
        g = np.load(p)
        sh = (g["xyz"] - g["box_min"]).astype(np.int32)
        img, _ = ctx.grid_picture(sh, extent=(g["box_max"] - g["box_min"]).astype(np.int32))
        out += [img, g["image"]]
    return out


def _urban_images(ctx, seeds=(11, 12), n=200_000, bin_=100):
    return [ctx.grid_picture(synth.shift_to_origin(synth.urban(n, seed=s)), bin=bin_)[0] for s in seeds]


def test_golden_rasters(gpu_ctx, tmp_path):
    _check_batch(gpu_ctx, _golden_images(gpu_ctx), tmp_path)


@pytest.mark.parametrize("k", [0, 2])
@pytest.mark.parametrize("s", [3, 5, 15])
def test_shapes(gpu_ctx, k, s, tmp_path):
    images = [ref.image_of_mask(m) for m in SHAPES.values()]
    _check_batch(gpu_ctx, images, tmp_path, iterations=k, kernel_size=s)


@pytest.mark.parametrize("bin_", [100, 37])
def test_urban_rasters(gpu_ctx, bin_, tmp_path):
    images = _urban_images(gpu_ctx, bin_=bin_)
    images.insert(1, ref.image_of_mask(SHAPES["rings"]))
    _check_batch(gpu_ctx, images, tmp_path)


def _narrow_ring_with_blob():
    """10 x 9: a ring whose hole (image rows 3..5) holds a blob, a few rows above the bottom frame."""
    m = np.zeros((9, 10), np.uint8)
    m[1:8, 1:9] = 1
    m[3:6, 3:7] = 0
    m[4, 4:6] = 1
    return m


def _wide(w=100, h=6, seed=0):
    rng = np.random.default_rng(seed)
    m = (rng.random((h, w)) < 0.25).astype(np.uint8)
    m[0, :] = 0  # a background first row: its N neighbour under a wrong width would be inside the narrow tile
    return m


@pytest.mark.parametrize("k", [0, 2])
def test_isolation_narrow_then_wide(gpu_ctx, k):
    narrow = _narrow_ring_with_blob()
    solo = ref.find_contours(narrow)
    assert len(solo.contours) == 1  # the blob in the hole is not external
    e = np.zeros((7, 7), np.uint8)
    orders = [[narrow, _wide()], [_wide(), narrow], [_wide(33, 4, 1), narrow, _wide(), narrow, _wide(250, 3, 2), e],
              [narrow, narrow, _wide(101, 2, 3), narrow, _wide(40, 12, 4)]]
    for masks in orders:
        imgs = [ref.image_of_mask(m) for m in masks]
        fps = _check_batch(gpu_ctx, imgs, iterations=k, kernel_size=3)
        for m, fp in zip(masks, fps):
            if m is narrow and k == 0:
                assert len(fp.contours) == 1


def test_empty_tiles_between_others(gpu_ctx, tmp_path):
    z = np.zeros((20, 30, 3))
    imgs = [z, ref.image_of_mask(SHAPES["nested"]), z, np.zeros((1, 1, 3)), z.copy(),
            ref.image_of_mask(SHAPES["comb"]), z]
    fps = _check_batch(gpu_ctx, imgs, tmp_path)
    assert [len(f.contours) for f in fps][::2] == [0, 0, 0, 0]


def test_two_thousand_small_tiles(gpu_ctx):
    rng = np.random.default_rng(2000)
    imgs = []
    for t in range(2000):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        img = np.zeros((h, w, 3))
        img[..., 1] = rng.random((h, w)) * 30 * (rng.random() < 0.9)
        imgs.append(img)
    fps = gpu_ctx.footprints_batch(imgs)
    for t in range(2000):
        _same(fps[t], gpu_ctx.footprints(imgs[t]), f"tile {t}")
    for t in range(0, 2000, 50):
        _same(fps[t], ref.footprints(imgs[t])[0], f"tile {t} against the restatement")


def test_reordering_does_not_change_a_tile(gpu_ctx):
    imgs = _golden_images(gpu_ctx)[:4] + [ref.image_of_mask(SHAPES[n]) for n in ("rings", "checker", "edges")]
    imgs.append(ref.image_of_mask(_narrow_ring_with_blob()))
    base = gpu_ctx.footprints_batch(imgs)
    rng = np.random.default_rng(5)
    for _ in range(3):
        perm = rng.permutation(len(imgs))
        got = gpu_ctx.footprints_batch([imgs[i] for i in perm])
        for j, i in enumerate(perm):
            _same(got[j], base[i], f"tile {i} at position {j}")


def test_info_totals_are_sums_of_the_solo_runs(gpu_ctx):
    imgs = [ref.image_of_mask(m) for m in SHAPES.values()] + _urban_images(gpu_ctx, seeds=(3,))
    fps = gpu_ctx.footprints_batch(imgs)
    solo = [gpu_ctx.footprints(im).info for im in imgs]
    inf = fps[0].info
    for key in ("fg_pixels", "border_states", "components"):
        assert inf[key] == sum(s[key] for s in solo), key
    assert inf["components"] == sum(len(f.contours) for f in fps)
    assert inf["ms_total"] > 0


def test_errors_name_the_tile_and_leave_the_context_usable(gpu_ctx):
    imgs = [ref.image_of_mask(SHAPES["rings"]), np.zeros((5, 5, 3))]
    for kw in ({"kernel_size": 4}, {"kernel_size": 17}, {"iterations": -1}, {"iterations": 17}, {"threshold": 256},
               {"threshold": -1}):
        with pytest.raises(BsError) as ei:
            gpu_ctx.footprints_batch(imgs, **kw)
        assert ei.value.status == -1
    L, h = gpu_ctx._L, gpu_ctx._h
    img = np.zeros(3 * 64, np.float64)
    co = np.zeros(4, np.int32)
    out = api.Contours()
    for w, hh, bad in (([2, 0, 3], [2, 2, 2], 1), ([2, 2, 3], [2, 2, -1], 2)):
        w = np.array(w, np.int32)
        hh = np.array(hh, np.int32)
        rc = L.bs_footprints_batch(h, img.ctypes.data, w.ctypes.data, hh.ctypes.data, 3, 10, 5, 2, None,
                                   api.C.byref(out), co.ctypes.data, None)
        assert rc == -1 and f"tile {bad}" in L.bs_last_error(h).decode()
    w = np.array([40000, 40000, 40000], np.int32)  # 4.8 * 10^9 pixels in all
    rc = L.bs_footprints_batch_dev(h, 1, w.ctypes.data, w.ctypes.data, 3, 10, 5, 2, None, api.C.byref(out),
                                   co.ctypes.data, None)
    assert rc == -2
    w = np.array([30000, 30000, 30000], np.int32)  # 2.7 * 10^9 pixels: the image total is checked first
    assert L.bs_footprints_batch_dev(h, 1, w.ctypes.data, w.ctypes.data, 3, 10, 5, 2, None, api.C.byref(out),
                                     co.ctypes.data, None) == -2
    w = np.array([2, 2, 2], np.int32)
    assert L.bs_footprints_batch_dev(h, 1, w.ctypes.data, w.ctypes.data, 3, 10, 5, 2, None, api.C.byref(out),
                                     None, None) == -1  # contour_offset is required
    _check_batch(gpu_ctx, imgs)


def test_end_to_end_device_chain(gpu_ctx, oracle, tmp_path):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(16)
    raw = [synth.urban(int(rng.integers(50_000, 150_000)), seed=100 + t) + rng.integers(-10 ** 6, 10 ** 6, 3).astype(np.int32)
           for t in range(16)]
    xyz, off = api.pack_tiles(raw)
    d = torch.from_numpy(xyz).cuda()
    gpu_ctx.shift_tiles_to_origin_dev(d.data_ptr(), off)
    box = gpu_ctx.tile_boxes_dev(d.data_ptr(), off)
    ext = box[:, 3:] - box[:, :3]
    w, h, po = api.grid_dims_batch(ext)
    img = torch.empty(3 * int(po[-1]), dtype=torch.float64, device="cuda")
    mask = torch.empty(int(po[-1]), dtype=torch.uint8, device="cuda")
    gpu_ctx.grid_picture_batch_dev(d.data_ptr(), off, ext, img.data_ptr())
    fps = gpu_ctx.footprints_batch_dev(img.data_ptr(), w, h, d_mask=mask.data_ptr())
    hmask = mask.cpu().numpy()
    for t in range(16):
        sh = synth.shift_to_origin(raw[t])
        simg, _ = gpu_ctx.grid_picture(sh, extent=sh.max(0))
        solo, smask = gpu_ctx.footprints(simg, return_mask=True)
        assert (fps[t].width, fps[t].height) == (w[t], h[t])
        _same(fps[t], solo, f"tile {t}")
        assert np.array_equal(hmask[po[t]:po[t + 1]].reshape(h[t], w[t]), smask)
        api.write_footprints_obj(fps[t], tmp_path / "batch.obj")
        api.write_footprints_obj(solo, tmp_path / "solo.obj")
        assert (tmp_path / "batch.obj").read_bytes() == (tmp_path / "solo.obj").read_bytes()
    himg = img.cpu().numpy()
    for t in (0, 5, 10, 15):  # the solo call is a batch of one: these tiles against the CPU references as well
        sh = synth.shift_to_origin(raw[t])
        oimg, _ = oracle.grid_picture(sh, extent=sh.max(0))
        assert np.array_equal(himg[3 * po[t]:3 * po[t + 1]].reshape(h[t], w[t], 3), oimg), f"tile {t}: raster"
        r, rmask = ref.footprints(oimg)
        _same(fps[t], r, f"tile {t} against the restatement")
        assert np.array_equal(hmask[po[t]:po[t + 1]].reshape(h[t], w[t]), rmask * 255)
