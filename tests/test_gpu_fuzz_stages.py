"""Stages 4-6 on the device against their CPU references, where hand-picked cases did not reach: the differential
fuzzer tests/tools/fuzz_stages.py (plain and as batches; tests/test_fuzz_stages_cpu.py asserts what its cases reach),
and directed tests of the branches it is there for -- the height histogram beyond its LDS bins, the quantisation on
its integer boundaries, a far unique maximum, non-finite pixels, the assignment at the int32 limits.  Every
comparison is ==."""
import os
import subprocess
import sys

import numpy as np
import pytest

from buildingsegment_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))
sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
sys.path.insert(0, os.path.join(HERE, "building_ref"))
import building_ref as bref  # noqa: E402
import fuzz_stages as F  # noqa: E402
import ref  # noqa: E402
from test_gpu_buildings import POINT_FIGURES, _same_points  # noqa: E402
from test_gpu_footprints import _same  # noqa: E402

pytestmark = pytest.mark.gpu

# about three times the wall time of each run, start of the process included, measured on an MI355X box: 5.3 s
# plain and 2.3 s with --batch (device and references together; the tool's own count is 4.6 s and 1.9 s)
PLAIN_TIMEOUT, BATCH_TIMEOUT = 16, 8


def _fuzz(extra, timeout):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "fuzz_stages.py"), "--cases",
                          str(F.GPU_TEST_CASES), "--seed", str(F.GPU_TEST_SEED)] + extra,
                         capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert f"done: {F.GPU_TEST_CASES} cases, 0 mismatches, 0 skipped" in out.stdout


def test_fuzz_stages_plain():
    _fuzz([], PLAIN_TIMEOUT)


def test_fuzz_stages_batch():
    _fuzz(["--batch"], BATCH_TIMEOUT)


def test_two_runs_of_a_case_give_identical_arrays(gpu_ctx, oracle):
    """the first case of every kind of cloud and image, and the first image of the large size class"""
    seen = set()
    for i in range(F.GPU_TEST_CASES):
        case, p = F.replay_case(F.GPU_TEST_SEED, i)
        key = (case["kind"], case["sub"].split("+")[0])
        if case["kind"] == "image" and case["ch1"].size > F.LARGE_IMAGE:
            key = "strides"
        if key in seen:
            continue
        seen.add(key)
        recs = []
        for _ in range(2):
            ck = F.Check()
            rec, _ = F.run_cloud(gpu_ctx, oracle, case, p, ck) if case["kind"] == "cloud" else F.run_image(gpu_ctx, case, p, ck)
            assert not ck.why, (i, ck.why)
            recs.append(rec)
        assert F.same_records(*recs), i
    assert "strides" in seen and len(seen) == len(F.CLOUD_KINDS) + len(F.IMAGE_KINDS) + 1


# ---- the height histogram beyond its LDS bins ----------------------------------------------------------------------

def _tall_cloud(n=40_000, top=5_000_000, seed=3):
    rng = np.random.default_rng(seed)
    z = top - rng.integers(0, top, n) // 3  # two thirds of the range are empty: the threshold lies far up
    z[:50] = rng.integers(0, 4096, 50)      # a few points in the LDS bins as well
    xyz = np.concatenate([rng.integers(0, 3000, (n, 2)), z[:, None]], 1)
    xyz[0], xyz[1] = (0, 0, 0), (2999, 2999, top)
    return np.ascontiguousarray(xyz.astype(np.int32))


@pytest.mark.parametrize("bh", [1, 7])
def test_tall_cloud_height_bins_beyond_lds(gpu_ctx, oracle, bh):
    import torch
    xyz = _tall_cloud()
    oimg, oth = oracle.grid_picture(xyz, bin_height=bh)
    assert oth / bh >= 100 * F.ZH_LDS and oth % bh == 0  # millions of bins; the scan ends far beyond the LDS bins
    img, th = gpu_ctx.grid_picture(xyz, bin_height=bh)
    assert th == oth and np.array_equal(img, oimg)
    ext = xyz.max(0).astype(np.int32)
    w, h = api.grid_dims(ext)
    d_xyz = torch.from_numpy(xyz).cuda()
    d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
    assert gpu_ctx.grid_picture_dev(d_xyz.data_ptr(), len(xyz), ext, d_img.data_ptr(), bin_height=bh) == oth
    assert np.array_equal(d_img.cpu().numpy(), oimg)
    # the middle tile of a batch: its bins start at the sum of the tiles before it (hoff + b)
    rng = np.random.default_rng(bh)
    low = [np.ascontiguousarray(rng.integers(0, 4000, (m, 3)).astype(np.int32)) for m in (3000, 70, 9000)]
    other = _tall_cloud(9000, 900_000, seed=8)
    tiles = [low[0], low[1], xyz, other, low[2]]
    res = gpu_ctx.grid_picture_batch(tiles, bin_height=bh)
    for t, (timg, tth) in zip(tiles, res):
        wimg, wth = oracle.grid_picture(t, bin_height=bh)
        assert tth == wth and np.array_equal(timg, wimg)
    assert res[2][1] == oth


def test_ground_threshold_on_the_last_lds_bin_and_the_first_after(gpu_ctx, oracle):
    """the median exactly in bin 4095 and in bin 4096: the two sides of the histogram's split"""
    for b in (F.ZH_LDS - 1, F.ZH_LDS):
        z = np.concatenate([np.arange(0, 40), np.full(60, b * 10 + 3), np.arange(b * 10 + 10, b * 10 + 50)])
        xyz = np.ascontiguousarray(np.stack([np.arange(len(z)) * 7 % 500, np.arange(len(z)) * 13 % 400, z], 1).astype(np.int32))
        oimg, oth = oracle.grid_picture(xyz, bin_height=10)
        assert oth == b * 10
        img, th = gpu_ctx.grid_picture(xyz, bin_height=10)
        assert th == oth and np.array_equal(img, oimg)


# ---- quantisation and threshold --------------------------------------------------------------------------------------

def _check(ctx, img, **kw):
    fp, mask = ctx.footprints(img, return_mask=True, **kw)
    r, rmask = ref.footprints(img, **kw)
    assert np.array_equal(mask, rmask * 255), kw
    _same(fp, r)
    return rmask


def _check_batch(ctx, images, **kw):
    fps, masks = ctx.footprints_batch(images, return_mask=True, **kw)
    for img, fp, mask in zip(images, fps, masks):
        r, rmask = ref.footprints(img, **kw)
        assert np.array_equal(mask, rmask * 255), kw
        _same(fp, r)


def _real_image(h=211, w=317, seed=5, mx=27.43):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ch = np.maximum(np.sin(xx / 17.0) * np.cos(yy / 11.0) + 0.3 * rng.random((h, w)), 0) * mx
    return F.full_image(np.ascontiguousarray(ch))


def test_threshold_sweep_on_a_real_valued_image(gpu_ctx):
    img = _real_image()
    sums = []
    for thr in (0, 1, 10, 128, 254, 255):
        for it in (0, 2):
            _check(gpu_ctx, img, threshold=thr, iterations=it)
        sums.append(int(ref.mask(img, thr).sum()))
    assert sums == sorted(sums, reverse=True) and len(set(sums)) == 6 and sums[-1] == 0 and sums[-2] > 0
    assert not np.array_equal(ref.mask(img, 0).astype(bool), img[..., 1] != 0)  # q == 0 for small positive values
    _check_batch(gpu_ctx, [img, _real_image(40, 61, 6), img[:100]], threshold=128)
    _check_batch(gpu_ctx, [_real_image(40, 61, 6), img], threshold=254, iterations=0)


def _boundary_rows(mx, w=96):
    """every max * j / 255 with both neighbours, zeros between them (no two touch in a row, empty rows between the
    rows); the maximum in the last corner"""
    x = mx * np.arange(256) / 255.0
    trip = np.clip(np.stack([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)], 1).ravel(), 0.0, mx)
    cells = np.zeros(2 * len(trip))
    cells[::2] = trip
    rows = np.zeros((-(-len(cells) // w), w))
    rows.ravel()[:len(cells)] = cells
    ch = np.zeros((2 * len(rows) + 1, w))
    ch[:-1:2] = rows
    ch[-1, -1] = mx
    return F.full_image(ch), trip


@pytest.mark.parametrize("mx", [255.0, 1.0, 27.43, 1e-300, 1e300, 3e-320], ids=str)
def test_integer_boundary_rows_at_every_threshold(gpu_ctx, mx):
    img, trip = _boundary_rows(mx)
    q = F.quantised(img[..., 1])
    on = [(q == t).any() and (q == t + 1).any() for t in range(255)]
    assert all(on)  # every threshold has a pixel on it and one just above
    for thr in range(256):
        fp, mask = gpu_ctx.footprints(img, threshold=thr, kernel_size=1, iterations=0, return_mask=True)
        assert np.array_equal(mask, (q > thr) * np.uint8(255)), thr
        assert np.array_equal(mask, ref.mask(img, thr) * 255), thr
    for thr in (0, 1, 100, 127, 128, 254, 255):
        _check(gpu_ctx, img, threshold=thr, iterations=1)
        _check_batch(gpu_ctx, [img[:7], img, img[::-1].copy()], threshold=thr, iterations=0)


def _unique_max(h, w, at, seed=1, mx=30.0):
    rng = np.random.default_rng(seed)
    ch = np.where(rng.random((h, w)) < 0.3, rng.random((h, w)) * (0.5 * mx), 0.0)
    ch.ravel()[at] = mx
    return F.full_image(ch)


@pytest.mark.parametrize("where", ["first", "last"])
def test_unique_maximum_in_one_far_pixel(gpu_ctx, where):
    """3001 x 4093 pixels are 2999 blocks of max_tiled_kernel; with the maximum missed every q doubles"""
    h, w = 3001, 4093
    img = _unique_max(h, w, 0 if where == "first" else h * w - 1)
    for thr in (64, 127):
        rmask = _check(gpu_ctx, img, threshold=thr, iterations=0)
        assert 0 < rmask.sum() < h * w // 4
    # the same as tile 0 and as the last tile of a batch (max_tiled_kernel: blocks of 4096 pixels of one tile)
    a, b = _unique_max(301, 409, 0, 2), _unique_max(333, 260, 333 * 260 - 1, 3)
    mid = [_unique_max(50, 70, 1234, 4, mx=1e300), np.zeros((9, 9, 3)), _unique_max(64, 64, 4095, 5, mx=1e-300)]
    for tiles in ([a] + mid + [b], [b] + mid + [a]):
        _check_batch(gpu_ctx, tiles, threshold=127, iterations=0)
        _check_batch(gpu_ctx, tiles, threshold=64)


SPECIAL = {"negative": -3.5, "minus_zero": -0.0, "nan": np.nan, "plus_inf": np.inf, "minus_inf": -np.inf,
           "subnormal": 5e-324, "minus_huge": -1e308}


@pytest.mark.parametrize("name", list(SPECIAL) + ["all_but_plus_inf", "only_non_positive"])
def test_non_finite_and_negative_pixels(gpu_ctx, name):
    img = _real_image(90, 130, 9)
    rng = np.random.default_rng(len(name))
    at = rng.choice(img.shape[0] * img.shape[1], 400, replace=False)
    if name == "all_but_plus_inf":
        vals = rng.choice([v for k, v in SPECIAL.items() if k != "plus_inf"], len(at))
    elif name == "only_non_positive":
        img[..., 1] = -np.abs(img[..., 1])
        vals = rng.choice([np.nan, -np.inf, -0.0, 0.0], len(at))
    else:
        vals = np.full(len(at), SPECIAL[name])
    img[..., 1].ravel()[at] = vals
    img[0, 0, 1], img[-1, -1, 1] = vals[0], vals[-1]
    for thr in (0, 10, 200):
        rmask = _check(gpu_ctx, img, threshold=thr, iterations=1)
        if name in ("plus_inf", "only_non_positive"):
            assert rmask.sum() == 0  # max = inf: every quotient is 0 or NaN; max = 0: nothing is quantised
        else:
            assert rmask.sum() > 0
    _check_batch(gpu_ctx, [_real_image(30, 40, 2), img, _real_image(20, 70, 3)], threshold=10)
    sub = F.full_image(np.full((20, 30), 3e-320) * (np.random.default_rng(1).random((20, 30)) < 0.5))
    assert _check(gpu_ctx, sub, threshold=254, iterations=0).sum() > 0  # a subnormal maximum is a maximum


# ---- assignment ----------------------------------------------------------------------------------------------------

def _two_buildings():
    m = np.zeros((40, 90), np.uint8)
    m[5:35, 3:40] = 1
    m[10:30, 50:85] = 1
    return m


@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 5 + 17, 4096 + 63])
def test_assignment_edges(gpu_ctx, n):
    """z at the int32 limits (z_sum wraps through unsigned 64-bit sums on the device), negative and fractional
    thresholds, thresholds equal to a z, fewer points than a wave, and whole waves plus a partial one in a building"""
    bmap, b = gpu_ctx.building_map(_two_buildings() * 255)
    assert b.n_buildings == 2
    rng = np.random.default_rng(n)
    lim = np.array([F.I32_MIN, F.I32_MIN + 1, F.I32_MAX, F.I32_MAX - 1, -1, 0, 1, 1000], np.int64)
    for layout in ("one_building", "mixed", "outside"):
        if layout == "one_building":  # every wave, the partial last one as well, in one building
            xy = np.stack([rng.integers(50 * 7, 85 * 7, n), rng.integers(10 * 7, 30 * 7, n)], 1)
        elif layout == "mixed":
            xy = np.stack([rng.integers(0, 90 * 7, n), rng.integers(0, 40 * 7, n)], 1)
        else:
            xy = np.stack([rng.integers(41 * 7, 49 * 7, n), rng.integers(0, 40 * 7, n)], 1)
        for zs in ("limits", "max_only", "min_only"):
            z = {"limits": rng.choice(lim, n), "max_only": np.full(n, F.I32_MAX), "min_only": np.full(n, F.I32_MIN)}[zs]
            xyz = np.ascontiguousarray(np.concatenate([xy, z[:, None]], 1).astype(np.int32))
            for th in (float(F.I32_MIN), -2147483647.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1000.0, 2147483646.5, float(F.I32_MAX),
                       2147483648.0):
                bidx = gpu_ctx.assign_buildings(xyz, bmap, b, bin=7, ground_th=th)
                a = bref.assign(xyz, bmap, 2, 7, th)
                _same_points(bidx, b, a)
                if layout == "one_building":
                    assert b.n_points.tolist() == [0, n] or b.n_points.tolist() == [n, 0]
        if layout == "one_building" and n > 1:
            assert abs(int(b.z_sum.sum())) <= n * 2**31  # (the wrapped sums came back as signed 64-bit values)


def test_whole_and_partial_waves_in_buildings_beyond_the_lds_tables(gpu_ctx):
    """400 buildings, 64 or 65 consecutive points in each: whole waves of one building on both sides of FIG_CAP, and
    waves that straddle two buildings"""
    m = np.zeros((20 * 3 + 1, 20 * 3 + 1), np.uint8)
    m[1::3, 1::3] = 1
    bmap, b = gpu_ctx.building_map(m * 255)
    assert b.n_buildings == 400 > F.FIG_CAP
    ys, xs = np.nonzero(m)
    rng = np.random.default_rng(4)
    for per in (64, 65, 128):
        xy = np.repeat(np.stack([xs, ys], 1) * 5, per, axis=0) + rng.integers(0, 5, (400 * per, 2))
        z = rng.integers(-3000, 9000, len(xy))
        xyz = np.ascontiguousarray(np.concatenate([xy, z[:, None]], 1).astype(np.int32))
        for th in (0.0, 100000.0):
            bidx = gpu_ctx.assign_buildings(xyz, bmap, b, bin=5, ground_th=th)
            _same_points(bidx, b, bref.assign(xyz, bmap, 400, 5, th))
            assert (b.n_points == per).all()


def test_assignment_counts_points_equal_to_the_threshold_as_above(gpu_ctx):
    bmap, b = gpu_ctx.building_map(_two_buildings() * 255)
    n = 1000
    xyz = np.ascontiguousarray(np.stack([np.full(n, 60 * 7), np.full(n, 20 * 7), np.arange(n) % 10 * 250], 1).astype(np.int32))
    for th in (0.0, 250.0, 1000.0, 2250.0, 2250.5):
        bidx = gpu_ctx.assign_buildings(xyz, bmap, b, bin=7, ground_th=th)
        a = bref.assign(xyz, bmap, 2, 7, th)
        _same_points(bidx, b, a)
        assert b.n_above.sum() == (xyz[:, 2] >= th).sum()
    for k in POINT_FIGURES:
        assert getattr(b, k).shape == (2,)
