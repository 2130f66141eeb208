"""Footprint contours on the device (bs_footprints[_dev]) against the sequential restatement
tests/footprint_ref/contour_ref.c, scipy's morphology and labelling, and the reference's own density PNGs."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from buildingsegment_amd import api, synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
import ref  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "raster_*.npz")))
pytestmark = pytest.mark.gpu


def _scipy_close(m, s=5, k=2):
    import scipy.ndimage as nd
    st = ref.ellipse(s).astype(bool)
    if k == 0:
        return m.astype(bool)
    d = nd.binary_dilation(m.astype(bool), st, iterations=k, border_value=0)
    return nd.binary_erosion(d, st, iterations=k, border_value=1)


def _same(fp, r, tmp_path=None):
    assert len(fp.contours) == len(r.contours)
    for a, b in zip(fp.contours, r.contours):
        assert np.array_equal(a, b)
    assert np.array_equal(fp.area, r.area)
    assert np.array_equal(fp.perimeter, r.perimeter)
    if tmp_path is not None:
        api.write_footprints_obj(fp, tmp_path / "dev.obj")
        r.write_obj(tmp_path / "ref.obj")
        assert (tmp_path / "dev.obj").read_bytes() == (tmp_path / "ref.obj").read_bytes()


def _check_image(ctx, img, tmp_path=None, **kw):
    fp, mask = ctx.footprints(img, return_mask=True, **kw)
    r, rmask = ref.footprints(img, **kw)
    assert np.array_equal(mask, rmask * 255)
    _same(fp, r, tmp_path)
    return fp


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_mask_pinned_to_reference_png(gpu_ctx, path, tmp_path):
    g = np.load(path)
    sh = (g["xyz"] - g["box_min"]).astype(np.int32)
    ext = (g["box_max"] - g["box_min"]).astype(np.int32)
    img, _ = gpu_ctx.grid_picture(sh, extent=ext)
    _, mask = gpu_ctx.footprints(img, iterations=0, return_mask=True)
    assert np.array_equal(mask == 255, g["png_density"][..., 1] > 10)
    _check_image(gpu_ctx, img, tmp_path)           # and the whole stage on the device raster
    _check_image(gpu_ctx, g["image"], tmp_path)    # and on the reference's own raster


SIZES = [(1, 1), (63, 63), (64, 64), (65, 65), (15, 63), (17, 65), (16, 64), (33, 129), (1, 300), (300, 1),
         (3001, 4093)]


@pytest.mark.parametrize("shape", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("s,k", [(5, 2), (3, 1), (7, 3), (15, 1), (1, 2)])
def test_closing_matches_scipy(gpu_ctx, shape, s, k):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31 + s * 5 + k)
    m = rng.random(shape) < 0.3
    if shape[0] > 8 and shape[1] > 8:
        m[shape[0] // 3:shape[0] // 2, :] = True  # structure reaching both edges
    _, mask = gpu_ctx.footprints(ref.image_of_mask(m), kernel_size=s, iterations=k, return_mask=True)
    assert np.array_equal(mask == 255, _scipy_close(m, s, k))


def _rings(n=96):
    m = np.zeros((n, n), np.uint8)
    for k in range(0, n // 2, 4):
        m[k + 1:n - k - 1, k + 1:n - k - 1] = 1
        m[k + 3:n - k - 3, k + 3:n - k - 3] = 0
    return m


def _spiral(n):
    """A 1-pixel-wide square spiral with 1-pixel gaps: one component whose trace is ~n*n steps long."""
    m = np.zeros((n, n), np.uint8)
    x0, y0, x1, y1 = 1, 1, n - 2, n - 2
    while x1 - x0 >= 4 and y1 - y0 >= 4:
        m[y0, x0:x1 + 1] = 1
        m[y0:y1 + 1, x1] = 1
        m[y1, x0:x1 + 1] = 1
        m[y0 + 2:y1 + 1, x0] = 1
        m[y0 + 2, x0:x0 + 3] = 1  # step in to the next turn
        x0, y0, x1, y1 = x0 + 2, y0 + 2, x1 - 2, y1 - 2
    return m


def _comb(w):
    """Teeth one pixel wide and apart on a base row: the outer contour turns at every pixel."""
    m = np.zeros((2, w), np.uint8)
    m[1] = 1
    m[0, ::2] = 1
    return m


def _shapes():
    rng = np.random.default_rng(17)
    out = {}
    for i, (h, w, p) in enumerate([(200, 300, 0.05), (513, 257, 0.12), (64, 64, 0.4), (1000, 777, 0.02)]):
        out[f"blobs{i}"] = (rng.random((h, w)) < p).astype(np.uint8)
    out["rings"] = _rings()
    out["spiral"] = _spiral(257)
    out["comb"] = _comb(301)
    out["checker"] = (np.indices((70, 90)).sum(0) % 2).astype(np.uint8)
    e = np.zeros((50, 60), np.uint8)
    e[0:10, 0:60] = 1
    e[20:50, 0:5] = 1
    e[30:50, 50:60] = 1
    e[45:50, 20:30] = 1
    out["edges"] = e
    nest = _rings(64)
    nest[28:36, 28:36] = 1
    out["nested"] = nest
    return out


SHAPES = _shapes()


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("k", [0, 2])
def test_contours_match_restatement(gpu_ctx, name, k, tmp_path):
    _check_image(gpu_ctx, ref.image_of_mask(SHAPES[name]), tmp_path, iterations=k)


@pytest.mark.parametrize("n,bin_", [(400_000, 100), (400_000, 37)])
def test_urban_rasters(gpu_ctx, n, bin_, tmp_path):
    xyz = synth.shift_to_origin(synth.urban(n, seed=11))
    img, _ = gpu_ctx.grid_picture(xyz, bin=bin_)
    fp = _check_image(gpu_ctx, img, tmp_path)
    assert len(fp.contours) >= 1 and fp.info["fg_pixels"] > 1000


@pytest.mark.parametrize("column", [False, True], ids=["row", "column"])
@pytest.mark.parametrize("npix", [1, 4095, 4096, 4097, 8193])
def test_chunks_of_the_segmented_maximum(gpu_ctx, npix, column):
    """A block of the maximum takes 4096 pixels.  Under the true maximum (400, in the last pixel) every other pixel
    quantises to 9, background at threshold 10; a maximum that missed the last block would make them all foreground."""
    img = np.zeros((npix, 1, 3) if column else (1, npix, 3))
    img[..., 1] = 15.0
    img.reshape(-1, 3)[-1, 1] = 400.0
    fp = _check_image(gpu_ctx, img, iterations=0, threshold=10)
    last = [0, npix - 1] if column else [npix - 1, 0]
    assert len(fp.contours) == 1 and fp.contours[0].tolist() == [last]


@pytest.mark.parametrize("h", [15, 16, 17])
@pytest.mark.parametrize("w", [63, 64, 65])
def test_block_edges_of_the_closing(gpu_ctx, w, h):
    """A closing block writes 64 x 16 pixels: one block less a row / column, exactly one, and one more."""
    m = np.random.default_rng(64 * 16).random((h, w)) < 0.5
    _check_image(gpu_ctx, ref.image_of_mask(m.astype(np.uint8)), iterations=2, kernel_size=5)


def test_batch_and_solo_calls_alternate_on_one_context(gpu_ctx):
    """The solo call is a batch of one in the same scratch: no descriptor or buffer layout of the other tile count
    may survive into the next call."""
    rng = np.random.default_rng(65 * 17)
    tiles = [ref.image_of_mask(m) for m in list(SHAPES.values())[:7]]
    mid = ref.image_of_mask((rng.random((17, 65)) < 0.5).astype(np.uint8))
    one = ref.image_of_mask(np.ones((1, 1), np.uint8))
    want = [ref.footprints(im) for im in tiles]

    def batch():
        fps, masks = gpu_ctx.footprints_batch(tiles, return_mask=True)
        for fp, mask, (r, rmask) in zip(fps, masks, want):
            assert np.array_equal(mask, rmask * 255)
            _same(fp, r)

    batch()
    _check_image(gpu_ctx, mid)
    batch()
    fp = _check_image(gpu_ctx, one)
    assert len(fp.contours) == 1 and fp.contours[0].tolist() == [[0, 0]]


def _external_components(m):
    """First pixels (x, y), ascending in raster order, of the external 8-connected components, by scipy.ndimage.label."""
    import scipy.ndimage as nd
    p = np.pad(m != 0, 1)
    fg, _ = nd.label(p, structure=np.ones((3, 3)))
    bg, _ = nd.label(~p, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    flat = fg.ravel()
    idx = np.flatnonzero(flat)
    _, first = np.unique(flat[idx], return_index=True)
    starts = idx[first]
    wp = p.shape[1]
    ext = sorted(int(s) for s in starts if bg.ravel()[s - wp] == bg[0, 0])
    return [((s % wp) - 1, (s // wp) - 1) for s in ext]


@pytest.mark.parametrize("name", ["blobs0", "blobs1", "blobs3", "rings", "nested", "checker", "edges"])
def test_counts_and_start_pixels_independent(gpu_ctx, name):
    m = SHAPES[name]
    fp = gpu_ctx.footprints(ref.image_of_mask(m), iterations=0)
    starts = _external_components(m)
    assert len(fp.contours) == len(starts)
    assert [tuple(c[0]) for c in fp.contours] == starts[::-1]


def test_long_trace_spiral(gpu_ctx, tmp_path):
    m = _spiral(4096)
    fp = _check_image(gpu_ctx, ref.image_of_mask(m), tmp_path, iterations=0)
    assert len(fp.contours) == 1
    assert fp.info["border_states"] > 8 * 10**6 and 2 * int(m.sum()) > 10**6  # trace ~ twice the pixel count
    assert len(fp.contours[0]) < 20_000  # only the corners are emitted


def test_long_emission_comb(gpu_ctx, tmp_path):
    m = _comb(1_200_001)
    fp = _check_image(gpu_ctx, ref.image_of_mask(m), None, iterations=0)
    assert len(fp.contours) == 1 and len(fp.contours[0]) > 10**6


def test_large_image_16k(gpu_ctx):
    import torch
    rng = np.random.default_rng(23)
    h = w = 16_384
    coarse = rng.random((h // 16, w // 16)) < 0.3
    m = np.kron(coarse, np.ones((16, 16), bool))
    m &= rng.random((h, w)) < 0.97  # speckle: many small holes and isolated components
    mt = torch.from_numpy(m).cuda()
    img = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    img[..., 1] = mt.to(torch.float64) * 30.0
    del mt
    fp = gpu_ctx.footprints_dev(img.data_ptr(), w, h, iterations=0)
    del img
    torch.cuda.empty_cache()
    r = ref.find_contours(m)
    _same(fp, r)


def test_deterministic(gpu_ctx):
    img = ref.image_of_mask(SHAPES["blobs1"])
    a = gpu_ctx.footprints(img)
    b = gpu_ctx.footprints(img)
    _same(a, ref.footprints(img)[0])
    assert len(a.contours) == len(b.contours) and all(np.array_equal(x, y) for x, y in zip(a.contours, b.contours))
    assert np.array_equal(a.area, b.area) and np.array_equal(a.perimeter, b.perimeter)


def test_errors_and_empty(gpu_ctx):
    img = ref.image_of_mask(SHAPES["blobs0"])
    for kw in [dict(kernel_size=4), dict(kernel_size=0), dict(kernel_size=17), dict(iterations=-1),
               dict(iterations=17), dict(threshold=-1), dict(threshold=256)]:
        with pytest.raises(api.BsError) as e:
            gpu_ctx.footprints(img, **kw)
        assert e.value.status == -1
    with pytest.raises(api.BsError) as e:  # null image
        gpu_ctx.footprints_dev(0, 10, 10)
    assert e.value.status == -1
    with pytest.raises(api.BsError) as e:
        gpu_ctx.footprints_dev(1, 0, 10)
    assert e.value.status == -1
    with pytest.raises(api.BsError) as e:  # (w + 2) * (h + 2) >= 2^31
        gpu_ctx.footprints_dev(1, 65536, 32768)
    assert e.value.status == -1
    fp = gpu_ctx.footprints(np.zeros((40, 50, 3)))
    assert fp.contours == [] and fp.info["components"] == 0


def test_cli_writes_the_same_obj(gpu_ctx, tmp_path):
    from test_host_ply import write_ply
    exe = os.path.join(ROOT, "host", "tmc3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")])
    xyz = synth.urban(60_000, seed=5).astype(np.int64) + np.array([4321, 99, -20])
    src, dst, obj = str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), str(tmp_path / "cli.obj")
    metres = (xyz + np.where(xyz >= 0, 0.5, -0.5)) / 1000.0
    write_ply(src, metres, np.zeros((len(xyz), 3), np.uint8))
    res = subprocess.run([exe, "-a=" + src, "-s=" + dst, "--footprints=" + obj], capture_output=True, text=True,
                         check=True)
    assert "footprint contours" in res.stderr
    shifted = (xyz - xyz.min(0)).astype(np.int32)
    img, _ = gpu_ctx.grid_picture(shifted)
    fp = gpu_ctx.footprints(img)
    api.write_footprints_obj(fp, tmp_path / "py.obj")
    assert open(obj, "rb").read() == (tmp_path / "py.obj").read_bytes()
    assert len(fp.contours) > 0
