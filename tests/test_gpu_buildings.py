"""Buildings on the device (bs_building_map, bs_assign_buildings, bs_plane_buildings; include/bs_api.h) against the
numpy / scipy restatement tests/building_ref and against the contours of bs_footprints on the same mask.  Everything
is an exact integer: every comparison is ==."""
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
sys.path.insert(0, os.path.join(HERE, "building_ref"))
import building_ref as bref  # noqa: E402
import ref  # noqa: E402
import scenes  # noqa: E402
from test_gpu_footprints import SHAPES, SIZES, _spiral  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "raster_*.npz")))
pytestmark = pytest.mark.gpu

PIXEL_FIGURES, POINT_FIGURES = bref.PIXEL_FIGURES, bref.POINT_FIGURES


def _same_map(bmap, b, r):
    assert b.n_buildings == r.n_buildings and (b.width, b.height) == (r.width, r.height)
    assert np.array_equal(bmap, r.map)
    for k in PIXEL_FIGURES:
        assert np.array_equal(getattr(b, k), getattr(r, k)), k
    assert (b.n_points == 0).all() and (b.n_above == 0).all() and (b.z_sum == 0).all()
    assert (b.z_min == bref.I32_MAX).all() and (b.z_max == bref.I32_MIN).all()


def _same_contours(bmap, b, fp):
    """building c is contour c"""
    assert b.n_buildings == len(fp.contours)
    for c, pts in enumerate(fp.contours):
        assert tuple(pts[0]) == tuple(b.start_xy[c])
        assert (bmap[pts[:, 1], pts[:, 0]] == c).all()


def _check_mask(ctx, m):
    """the map of the 0 / 1 mask m against the restatement and the device contours of the same mask"""
    m = np.ascontiguousarray(np.asarray(m) != 0, dtype=np.uint8)
    bmap, b = ctx.building_map(m * 255)
    _same_map(bmap, b, bref.building_map(m))
    _same_contours(bmap, b, ctx.footprints(ref.image_of_mask(m), iterations=0))
    return bmap, b


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("k", [0, 2])
def test_map_of_shapes(gpu_ctx, name, k):
    fp, mask = gpu_ctx.footprints(ref.image_of_mask(SHAPES[name]), iterations=k, return_mask=True)
    bmap, b = gpu_ctx.building_map(mask)  # the closed mask exactly as bs_footprints writes it (0 / 255)
    _same_map(bmap, b, bref.building_map(mask))
    _same_contours(bmap, b, fp)
    if name == "blobs3" and k == 0:
        assert b.n_buildings == 14330


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_map_of_golden_rasters(gpu_ctx, path):
    fp, mask = gpu_ctx.footprints(np.load(path)["image"], return_mask=True)
    bmap, b = gpu_ctx.building_map(mask)
    _same_map(bmap, b, bref.building_map(mask))
    _same_contours(bmap, b, fp)


# the padded grid is cut into 64 x 16 tiles: image sizes whose padded size is a tile edge, one less and one more
TILE_SIZES = [(13, 61), (14, 62), (15, 63), (14, 63), (15, 62), (29, 125), (30, 126), (31, 127), (46, 190), (14, 1000),
              (1000, 62), (47, 191)]


@pytest.mark.parametrize("shape", SIZES + TILE_SIZES, ids=[f"{h}x{w}" for h, w in SIZES + TILE_SIZES])
def test_map_of_random_masks_by_size(gpu_ctx, shape):
    rng = np.random.default_rng(shape[0] * 7919 + shape[1] * 31)
    for p in (0.3, 0.55):  # scattered blobs / one percolating mass with many holes
        m = rng.random(shape) < p
        if shape[0] > 8 and shape[1] > 8:
            m[shape[0] // 3:shape[0] // 2, :] = True  # structure reaching both edges
        _check_mask(gpu_ctx, m)


def test_map_of_the_spiral_crosses_every_seam(gpu_ctx):
    m = _spiral(4096)
    bmap, b = _check_mask(gpu_ctx, m)
    assert b.n_buildings == 1 and b.fg_pixels[0] == m.sum()
    assert b.bbox.tolist() == [[1, 1, 4094, 4094]] and b.start_xy.tolist() == [[1, 1]]


def test_map_all_foreground_and_empty(gpu_ctx):
    for shape in [(1, 1), (16, 64), (100, 300), (777, 1030)]:
        bmap, b = _check_mask(gpu_ctx, np.ones(shape, np.uint8))
        h, w = shape
        assert b.n_buildings == 1 and (bmap == 0).all() and b.pixels.tolist() == [h * w] == b.fg_pixels.tolist()
        assert b.bbox.tolist() == [[0, 0, w - 1, h - 1]]
        bmap, b = gpu_ctx.building_map(np.zeros(shape, np.uint8))
        assert b.n_buildings == 0 and (bmap == -1).all() and b.pixels.shape == (0,) and b.start_xy.shape == (0, 2)


def test_map_large_image_8k(gpu_ctx):
    import torch
    rng = np.random.default_rng(29)
    h, w = 8192, 8200
    coarse = rng.random((h // 8, w // 8)) < 0.33
    m = np.kron(coarse, np.ones((8, 8), bool))
    m &= rng.random((h, w)) < 0.97  # speckle: many small holes, and rings of blocks that enclose others
    d_mask = torch.from_numpy(m.astype(np.uint8)).cuda()
    d_map = torch.empty((h, w), dtype=torch.int32, device="cuda")
    b = gpu_ctx.building_map_dev(d_mask.data_ptr(), w, h, d_map.data_ptr())
    bmap = d_map.cpu().numpy()
    del d_map, d_mask
    torch.cuda.empty_cache()
    r = bref.building_map(m)
    _same_map(bmap, b, r)
    assert b.n_buildings > 1000 and (b.pixels > b.fg_pixels).sum() > 100
    d_img = torch.zeros((h, w, 3), dtype=torch.float64, device="cuda")
    d_img[..., 1] = torch.from_numpy(m).cuda().to(torch.float64) * 30.0
    fp = gpu_ctx.footprints_dev(d_img.data_ptr(), w, h, iterations=0)
    del d_img
    torch.cuda.empty_cache()
    _same_contours(bmap, b, fp)


def _same_points(bidx, b, a):
    assert np.array_equal(bidx, a.building_idx)
    for k in POINT_FIGURES:
        assert np.array_equal(getattr(b, k), getattr(a, k)), k


def _same_votes(v, want):
    for got, w, k in zip((v.plane_building, v.votes_in, v.votes_total, v.votes_outside), want,
                         ("plane_building", "votes_in", "votes_total", "votes_outside")):
        assert got.dtype == w.dtype and np.array_equal(got, w), k


@pytest.fixture(scope="module")
def composed(gpu_ctx):
    xyz = scenes.composed()
    _, _, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=16))
    return xyz, plane_idx, len(planes)


def test_composed_scene_assignment_and_votes(gpu_ctx, composed):
    xyz, plane_idx, n_planes = composed
    fp, b = gpu_ctx.buildings(xyz, plane_idx, n_planes)
    img, th = gpu_ctx.grid_picture(xyz)
    rfp, mask = gpu_ctx.footprints(img, return_mask=True)
    assert th == b.ground_th and len(rfp.contours) == len(fp.contours) == b.n_buildings
    r = bref.building_map(mask)
    _same_contours(b.map, b, fp)
    assert np.array_equal(b.map, r.map)
    for k in PIXEL_FIGURES:
        assert np.array_equal(getattr(b, k), getattr(r, k)), k
    a = bref.assign(xyz, r.map, r.n_buildings, 100, th)
    _same_points(b.building_idx, b, a)
    want = bref.votes(plane_idx, a.building_idx, n_planes, r.n_buildings)
    _same_votes(b.votes, want)
    # the kinds this scene is there for
    px, py = xyz[:, 0] // 100, xyz[:, 1] // 100
    assert b.n_buildings >= 8 and len(fp.kept()) >= 8
    assert (b.building_idx == -1).any() and not ((b.building_idx == -1) & a.above).any()
    assert bref.enclosed_pixels(mask, b.map)[py, px].any()  # the courtyard belongs to the ring
    v = b.votes
    assert ((v.votes_outside > 0) & (v.plane_building >= 0)).any()
    assert ((v.plane_building == -1) & (v.votes_total > 0)).any() and (v.votes_in[v.plane_building == -1] == 0).all()
    assert (v.votes_total == np.bincount(plane_idx[plane_idx > 0], minlength=n_planes + 1)[1:n_planes + 1]).all()


def test_composed_scene_device_pointers_and_point_order(gpu_ctx, composed):
    """the *_dev entry points, and the cloud sorted by building: whole waves in one building take the register path"""
    import torch
    xyz, plane_idx, n_planes = composed
    _, b0 = gpu_ctx.buildings(xyz, plane_idx, n_planes)
    order = np.argsort(b0.building_idx, kind="stable")
    for sel in (np.arange(len(xyz)), order):
        pts, pl = np.ascontiguousarray(xyz[sel]), np.ascontiguousarray(plane_idx[sel])
        d_xyz, d_pl = torch.from_numpy(pts).cuda(), torch.from_numpy(pl).cuda()
        ext = pts.max(0).astype(np.int32)
        w, h = api.grid_dims(ext)
        d_img = torch.empty((h, w, 3), dtype=torch.float64, device="cuda")
        th = gpu_ctx.grid_picture_dev(d_xyz.data_ptr(), len(pts), ext, d_img.data_ptr())
        d_mask = torch.empty((h, w), dtype=torch.uint8, device="cuda")
        fp = gpu_ctx.footprints_dev(d_img.data_ptr(), w, h, d_mask=d_mask.data_ptr())
        d_map = torch.empty((h, w), dtype=torch.int32, device="cuda")
        b = gpu_ctx.building_map_dev(d_mask.data_ptr(), w, h, d_map.data_ptr())
        d_bidx = torch.empty(len(pts), dtype=torch.int32, device="cuda")
        gpu_ctx.assign_buildings_dev(d_xyz.data_ptr(), len(pts), d_map.data_ptr(), b, d_bidx.data_ptr(), ground_th=th)
        v = gpu_ctx.plane_buildings_dev(d_pl.data_ptr(), d_bidx.data_ptr(), len(pts), n_planes, b.n_buildings)
        assert np.array_equal(d_map.cpu().numpy(), b0.map) and th == b0.ground_th
        _same_contours(b0.map, b, fp)
        for k in PIXEL_FIGURES + POINT_FIGURES:
            assert np.array_equal(getattr(b, k), getattr(b0, k)), k
        assert np.array_equal(d_bidx.cpu().numpy(), b0.building_idx[sel])
        _same_votes(v, (b0.votes.plane_building, b0.votes.votes_in, b0.votes.votes_total, b0.votes.votes_outside))
        assert b.info["ms_assign"] > 0 and b.info["ms_label_mask"] > 0


def _above_ground_is_assigned(ctx, xyz, bin_):
    img, th = ctx.grid_picture(xyz, bin=bin_)
    _, mask = ctx.footprints(img, return_mask=True)
    bmap, b = ctx.building_map(mask)
    bidx = ctx.assign_buildings(xyz, bmap, b, bin=bin_, ground_th=th)
    a = bref.assign(xyz, bmap, b.n_buildings, bin_, th)
    _same_points(bidx, b, a)
    assert a.above.any() and (bidx[a.above] >= 0).all()
    assert b.n_above.sum() == a.above.sum()


@pytest.mark.parametrize("bin_", [100, 37])
def test_above_ground_points_are_assigned_urban(gpu_ctx, bin_):
    _above_ground_is_assigned(gpu_ctx, synth.shift_to_origin(synth.urban(400_000, seed=11)), bin_)


def test_above_ground_points_are_assigned_composed(gpu_ctx, composed):
    _above_ground_is_assigned(gpu_ctx, composed[0], 100)


def _random_points(m, n, bin_, seed):
    rng = np.random.default_rng(seed)
    h, w = m.shape
    return np.stack([rng.integers(0, w * bin_, n), rng.integers(0, h * bin_, n), rng.integers(-3000, 9000, n)],
                    1).astype(np.int32)


@pytest.mark.parametrize("n_planes", [5, 200, 2000], ids=["few_planes", "dense_histogram", "sorted_keys"])
@pytest.mark.parametrize("order", ["random", "by_pixel"])
def test_more_buildings_than_the_lds_tables(gpu_ctx, n_planes, order):
    """14 330 buildings: all but the first 256 take the global-atomic path of the figures.  5 / 200 / 2000 planes
    give a vote table of 7e4, 2.9e6 and 2.9e7 cells: a dense histogram in HBM twice, then sorted keys; with the
    building indices folded to 3 buildings every table fits the workgroup-private histogram."""
    m = SHAPES["blobs3"]
    bmap, b = gpu_ctx.building_map(m * 255)
    assert b.n_buildings == 14330
    xyz = _random_points(m, 600_000, 7, 5)
    if order == "by_pixel":  # 64 consecutive points in one pixel: whole waves in one building
        xyz = xyz[np.argsort((xyz[:, 1] // 7) * m.shape[1] + xyz[:, 0] // 7, kind="stable")]
        xyz = np.ascontiguousarray(np.repeat(xyz[::64], 64, axis=0)[:len(xyz)])
        xyz[:, 2] += (np.arange(len(xyz)) % 64).astype(np.int32) * 40
    bidx = gpu_ctx.assign_buildings(xyz, bmap, b, bin=7, ground_th=500.0)
    a = bref.assign(xyz, bmap, b.n_buildings, 7, 500.0)
    _same_points(bidx, b, a)
    assert (bidx >= 256).any() and ((bidx >= 0) & (bidx < 256)).any() and (bidx == -1).any()
    plane = np.random.default_rng(n_planes).integers(-1, n_planes + 3, len(xyz)).astype(np.int32)
    plane[plane == 0] = -1
    nb = b.n_buildings
    for nb_, bi in ((nb, bidx), (3, np.where(bidx < 3, bidx, -1).astype(np.int32))):
        v = gpu_ctx.plane_buildings(plane, bi, n_planes, nb_)
        want = bref.votes(plane, bi, n_planes, nb_)
        _same_votes(v, want)
    # ties are common here: the rule (lower index) is what decides many planes
    counts = np.zeros((n_planes, nb), np.int64)
    sel = (plane >= 1) & (plane <= n_planes) & (bidx >= 0)
    np.add.at(counts, (plane[sel] - 1, bidx[sel]), 1)
    if n_planes >= 200:
        assert ((counts == counts.max(1, keepdims=True)).sum(1)[counts.max(1) > 0] > 1).any()


def test_two_runs_give_identical_arrays(gpu_ctx, composed):
    xyz, plane_idx, n_planes = composed
    runs = [gpu_ctx.buildings(xyz, plane_idx, n_planes)[1] for _ in range(2)]
    m = SHAPES["blobs3"]
    pts = _random_points(m, 300_000, 7, 9)
    pl = np.random.default_rng(1).integers(1, 2001, len(pts)).astype(np.int32)
    extra = []
    for _ in range(2):
        bmap, b = gpu_ctx.building_map(m * 255)
        b.map = bmap
        b.building_idx = gpu_ctx.assign_buildings(pts, bmap, b, bin=7, ground_th=0.0)
        b.votes = gpu_ctx.plane_buildings(pl, b.building_idx, 2000, b.n_buildings)
        extra.append(b)
    for x, y in (runs, extra):
        assert np.array_equal(x.map, y.map) and np.array_equal(x.building_idx, y.building_idx)
        for k in PIXEL_FIGURES + POINT_FIGURES:
            assert np.array_equal(getattr(x, k), getattr(y, k)), k
        _same_votes(x.votes, (y.votes.plane_building, y.votes.votes_in, y.votes.votes_total, y.votes.votes_outside))


def test_errors_leave_the_context_usable(gpu_ctx):
    import torch
    m = SHAPES["blobs0"]
    h, w = m.shape
    bmap, b = gpu_ctx.building_map(m * 255)
    xyz = _random_points(m, 5000, 10, 3)
    good = gpu_ctx.assign_buildings(xyz, bmap, b, bin=10, ground_th=0.0)
    figures = {k: getattr(b, k).copy() for k in POINT_FIGURES}

    def raises(status, fn, *a, **kw):
        with pytest.raises(api.BsError) as e:
            fn(*a, **kw)
        assert e.value.status == status

    for bad in ([w * 10, 5, 0], [5, h * 10, 0], [-1, 5, 0], [5, -1, 0]):  # a pixel outside the image
        pts = xyz.copy()
        pts[1234] = bad
        raises(-2, gpu_ctx.assign_buildings, pts, bmap, b, bin=10, ground_th=0.0)
        for k in POINT_FIGURES:  # the figures are left as they were
            assert np.array_equal(getattr(b, k), figures[k])
    raises(-2, gpu_ctx.assign_buildings, xyz, bmap, b, bin=9, ground_th=0.0)  # a finer bin than the map's
    raises(-1, gpu_ctx.assign_buildings, xyz, bmap, b, bin=0)
    raises(-1, gpu_ctx.assign_buildings, xyz[:0], bmap, b, bin=10)
    d, d2 = (torch.zeros(64, dtype=torch.int32, device="cuda") for _ in range(2))
    p, p2 = d.data_ptr(), d2.data_ptr()
    raises(-1, gpu_ctx.building_map_dev, 0, 4, 4, p)
    raises(-1, gpu_ctx.building_map_dev, p, 4, 4, 0)
    raises(-1, gpu_ctx.building_map_dev, p, 0, 4, p)
    raises(-1, gpu_ctx.building_map_dev, p, 65536, 32768, p)  # (w + 2) * (h + 2) >= 2^31
    small = gpu_ctx.building_map_dev(p, 4, 4, p2)
    raises(-1, gpu_ctx.assign_buildings_dev, 0, 5, p, small, p, bin=1)
    raises(-1, gpu_ctx.assign_buildings_dev, p, 5, 0, small, p, bin=1)
    raises(-1, gpu_ctx.assign_buildings_dev, p, 5, p, small, 0, bin=1)
    raises(-1, gpu_ctx.assign_buildings_dev, p, 5, p, small, p, bin=0)
    raises(-1, gpu_ctx.plane_buildings_dev, 0, p, 5, 2, 0)
    raises(-1, gpu_ctx.plane_buildings_dev, p, 0, 5, 2, 0)
    raises(-1, gpu_ctx.plane_buildings_dev, p, p, 5, -1, 0)
    raises(-1, gpu_ctx.plane_buildings_dev, p, p, 5, 2, -1)
    raises(-1, gpu_ctx.plane_buildings, good, good, -1, b.n_buildings)
    raises(-2, gpu_ctx.plane_buildings, np.ones_like(good), good, 3, 1)  # building indices >= n_buildings
    assert gpu_ctx.plane_buildings(np.ones_like(good), good, 0, b.n_buildings).plane_building.shape == (0,)
    # and the context still works
    again = gpu_ctx.assign_buildings(xyz, bmap, b, bin=10, ground_th=0.0)
    assert np.array_equal(again, good)
    _same_points(again, b, bref.assign(xyz, bmap, b.n_buildings, 10, 0.0))
    _same_votes(gpu_ctx.plane_buildings(np.ones_like(good), good, 1, b.n_buildings),
                bref.votes(np.ones_like(good), good, 1, b.n_buildings))


@pytest.mark.parametrize("cloud", ["urban_60k", "boxes"])
def test_cli_writes_the_same_buildings_obj(gpu_ctx, tmp_path, cloud):
    from test_host_ply import write_ply
    exe = os.path.join(ROOT, "host", "tmc3")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "host")])
    if cloud == "urban_60k":  # the cloud of test_cli_writes_the_same_obj: part of one building, nothing is kept
        xyz = synth.urban(60_000, seed=5).astype(np.int64) + np.array([4321, 99, -20])
    else:  # four whole buildings of 4 to 6 m: all kept
        xyz = synth.boxes(n_boxes=4, edge_lo=80, edge_hi=120, pitch=9000).astype(np.int64) + np.array([-700, 123456, 30])
    src, dst, obj = str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), str(tmp_path / "cli.obj")
    metres = (xyz + np.where(xyz >= 0, 0.5, -0.5)) / 1000.0
    write_ply(src, metres, np.zeros((len(xyz), 3), np.uint8))
    res = subprocess.run([exe, "-a=" + src, "-s=" + dst, "--buildings=" + obj], capture_output=True, text=True,
                         check=True)
    assert "buildings" in res.stderr
    origin = xyz.min(0)
    shifted = (xyz - origin).astype(np.int32)
    _, _, plane_idx, planes = gpu_ctx.segment(shifted, api.default_params(k=15))
    fp, b = gpu_ctx.buildings(shifted, plane_idx, len(planes))
    api.write_buildings_obj(fp, b, tmp_path / "py.obj", origin=origin)
    got = open(obj, "rb").read()
    assert got == (tmp_path / "py.obj").read_bytes()
    assert got == bref.obj_text(fp.contours, fp.area, fp.perimeter, b.n_above, b.z_sum, 100, origin, b.ground_th)
    kept = [i for i in fp.kept() if b.n_above[i] > 0]
    assert len(fp.contours) > 0 and got.startswith(f"# buildings: {len(kept)} of {len(fp.contours)}\n".encode())
    if cloud == "boxes":
        assert len(kept) == 4 and got.count(b"\nf ") > 16
    won = int((b.votes.plane_building >= 0).sum())
    assert f"{len(planes)} planes, {won} with a building" in res.stderr
