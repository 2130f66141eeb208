"""Roofs on the device (bs_roofs, bs_roofs_dev; include/bs_api.h) against the numpy restatement tests/roof_ref.  The
one division apart, everything is an exact integer, and the division is the same IEEE operation on both sides: every
comparison is ==."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "building_ref"))
sys.path.insert(0, os.path.join(HERE, "roof_ref"))
import building_ref as bref  # noqa: E402
import fuzz_cases as fz  # noqa: E402
import roof_ref as rr  # noqa: E402
from test_roofs_cpu import check_gabled_facts, load_roof_scenes  # noqa: E402

pytestmark = pytest.mark.gpu
I32_MIN = rr.I32_MIN


def case(xyz, bmap, plane, n_planes, home=None, normal=None, center=None, bin=10, ground_th=0.0, min_votes=1):
    """a case dict as tests/roof_ref/fuzz_cases.py makes them; by default every plane is flat and at home in building 0"""
    if home is None:
        home = np.zeros(n_planes, np.int32)
    if normal is None:
        normal = np.tile([0.0, 0.0, 1.0], (n_planes, 1))
    if center is None:
        center = np.tile(np.array([0, 0, 100], np.int32), (n_planes, 1))
    return dict(xyz=np.asarray(xyz, np.int32).reshape(-1, 3), bmap=np.asarray(bmap, np.int32), plane_idx=np.asarray(plane, np.int32),
                n_planes=n_planes, home=np.asarray(home, np.int32), normal=np.asarray(normal, np.float64),
                center=np.asarray(center, np.int32), bin=bin, ground_th=ground_th, min_votes=min_votes)


def run(ctx, c, **kw):
    return ctx.roofs(c["xyz"], c["bmap"], c["plane_idx"], c["home"], c["normal"], c["center"], bin=c["bin"],
                     ground_th=c["ground_th"], min_votes=c["min_votes"], **kw)


def same(r, want, images=("roof", "support", "height")):
    for k in images:
        got = getattr(r, k)
        assert got.dtype == np.int32 and np.array_equal(got, getattr(want, k)), k
    same_figures(r, want)


def same_figures(r, want):
    assert r.n_planes == want.n_planes
    for k in rr.FIGURES:
        got = getattr(r, k)
        assert got.dtype == getattr(want, k).dtype and np.array_equal(got, getattr(want, k)), k
    for k in rr.TOTALS:
        assert getattr(r, k) == getattr(want, k), k


def check(ctx, c):
    r, want = run(ctx, c), fz.run_ref(c)
    same(r, want)
    return r


def pts(pixels, bin=10, z=50):
    """one point in the middle of every pixel (x, y)"""
    p = np.asarray(pixels, np.int64).reshape(-1, 2)
    return np.stack([p[:, 0] * bin + bin // 2, p[:, 1] * bin + bin // 2, np.full(len(p), z)], 1).astype(np.int32)


# ---- vote ----------------------------------------------------------------------------------------------------------
def test_vote_ties_homes_and_ignored_labels(gpu_ctx):
    bmap = np.array([[0, 0, 0, -1], [1, 1, 0, 0]], np.int32)
    home = np.array([0, 0, 1, 0], np.int32)
    px = [(0, 0)] * 6 + [(1, 0)] * 5 + [(3, 0)] * 3 + [(0, 1)] * 4 + [(2, 1)] * 6
    plane = [4, 4, 2, 2, 1, 4,      # pixel (0, 0): planes 4 and 2... 4 has three, 2 has two: 4 wins
             2, 4, 4, 2, 3,         # (1, 0): 2 and 4 tie with two each: the lower id; 3 is at home elsewhere
             1, 1, 1,               # (3, 0): a pixel outside every building
             1, 1, 1, 3,            # (0, 1) in building 1: plane 1 has most points but the wrong home, 3 wins with one
             0, -1, 5, 5, 5, 2]     # (2, 1): labels 0, -1 and n_planes + 1 are ignored: 2 wins with one
    c = case(pts(px), bmap, plane, 4, home)
    r = check(gpu_ctx, c)
    assert r.roof.tolist() == [[4, 2, 2, -1], [3, 3, 2, 2]] and r.support.tolist() == [[3, 2, 0, 0], [1, 0, 1, 0]]
    assert r.n_support.tolist() == [0, 3, 1, 3] and r.seeded_pixels == 4 and r.filled_pixels == 3 and r.unroofed_pixels == 0


def test_vote_ground_threshold_is_not_less_than(gpu_ctx):
    bmap = np.zeros((1, 4), np.int32)
    for th, zs, want in ((1000.0, [1000, 999, 1001, -5], [1, 0, 1, 0]), (1000.5, [1000, 1001, 1002, 999], [0, 1, 1, 0]),
                         (-3.0, [-3, -4, 0, -2], [1, 0, 1, 1])):
        xyz = pts([(0, 0), (1, 0), (2, 0), (3, 0)])
        xyz[:, 2] = zs
        c = case(xyz, bmap, [1, 1, 1, 1], 1, ground_th=th)
        r = check(gpu_ctx, c)
        assert r.support.tolist() == [want] and r.seeded_pixels == sum(want)


@pytest.mark.parametrize("min_votes", [1, 2, 5])
def test_vote_min_votes(gpu_ctx, min_votes):
    bmap = np.zeros((3, 7), np.int32)
    bmap[1] = -1  # row 2 is cut off from the seeds: what the threshold refuses there stays unroofed
    counts = [1, 2, 4, 5, 6, 1, 9]
    px = [(x, y) for y in (0, 2) for x, k in enumerate(counts) for _ in range(k)]
    plane = [1 + (i % 2 if x == 6 else 0) for y in (0, 2) for x, k in enumerate(counts) for i in range(k)]  # x == 6: 5 and 4
    c = case(pts(px), bmap, plane, 2, min_votes=min_votes)
    r = check(gpu_ctx, c)
    want = [k if k >= min_votes else 0 for k in counts[:6]] + [5 if min_votes <= 5 else 0]
    assert r.support[0].tolist() == want == r.support[2].tolist()
    assert r.seeded_pixels == 2 * sum(k > 0 for k in want) and r.unroofed_pixels == 0  # (the fill reaches the rest)


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_vote_all_points_in_one_pixel(gpu_ctx, n):
    bmap = np.zeros((3, 3), np.int32)
    xyz = np.tile(pts([(1, 1)]), (n, 1))
    xyz[:, 2] = 10 * np.arange(n) - 100
    c = case(xyz, bmap, np.where(np.arange(n) % 3 == 2, 1, 2), 2, ground_th=-50.0)
    r = check(gpu_ctx, c)
    above = np.arange(n)[10 * np.arange(n) - 100 >= -50]
    n1, n2 = int((above % 3 == 2).sum()), int((above % 3 != 2).sum())
    if n1 + n2:
        win = 2 if n2 > n1 else 1
        assert r.roof.tolist() == [[win] * 3] * 3 and r.support[1, 1] == max(n1, n2) and r.fill_rounds == 2
        assert r.n_support[win - 1] == max(n1, n2) and r.n_support[2 - win] == 0
    else:
        assert (r.roof == 0).all() and r.unroofed_pixels == 9 and r.fill_rounds == 0


# ---- fill ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("column", [False, True], ids=["row", "column"])
@pytest.mark.parametrize("n", [9, 64, 65, 129])
def test_fill_strip_meets_at_the_midpoint(gpu_ctx, n, column):
    bmap = np.zeros((1, n), np.int32)
    ends = [(0, 0), (n - 1, 0)]
    if column:
        bmap, ends = bmap.T.copy(), [(0, 0), (0, n - 1)]
    c = case(pts(ends), bmap, [5, 2], 5)
    r = check(gpu_ctx, c)
    x = np.arange(n)
    want = np.where(x < n - 1 - x, 5, 2)  # the middle pixel of an odd strip is reached by both in one round: the lower id
    assert r.roof.ravel().tolist() == want.tolist() and r.fill_rounds == (n - 1) // 2
    assert r.pixels[4] == n // 2 and r.pixels[1] == n - n // 2 and r.seeded_pixels == 2


def test_fill_goes_round_the_u_and_through_the_corridor(gpu_ctx):
    bmap = np.full((9, 11), -1, np.int32)
    bmap[:, 0] = bmap[:, 10] = bmap[8, :] = 0       # a U: two legs joined at the bottom
    bmap[0, 2:9] = 1                                 # another building between the tips
    c = case(pts([(0, 0), (3, 8), (4, 0)]), bmap, [3, 1, 2], 3, home=[0, 1, 0])
    r = check(gpu_ctx, c)
    # (10, 0), the tip of the right leg, is 10 pixels from the seed of plane 3 at (0, 0) and 10.6 from the seed of plane 1
    # at (3, 8) in the image, but 26 and 15 along the U: the nearer seed in the image is not the one that gets there
    assert r.roof[0, 10] == 1 and r.roof[0, 0] == 3 and (r.roof[0, 2:9] == 2).all()
    # down the left leg 3 reaches (0, y) in round y, 1 comes up from the bottom in round 3 + 8 - y
    assert r.roof[:, 0].tolist() == [3, 3, 3, 3, 3, 3, 1, 1, 1] and (r.roof[8] == 1).all() and (r.roof[:, 10] == 1).all()
    assert r.unroofed_pixels == 0 and r.fill_rounds == 15
    corridor = np.full((5, 40), -1, np.int32)
    corridor[2, :] = 0
    corridor[:, 39] = 0
    r = check(gpu_ctx, case(pts([(0, 2)]), corridor, [1], 1))
    assert (r.roof[corridor == 0] == 1).all() and r.fill_rounds == 39 + 2 and r.filled_pixels == 43


def test_fill_never_crosses_between_adjacent_buildings(gpu_ctx):
    bmap = np.zeros((6, 12), np.int32)
    bmap[:, 5:] = 1   # 4-adjacent along a whole column
    bmap[3:, 9:] = 2  # a third one without a seed of its own
    c = case(pts([(0, 0), (11, 0), (4, 5)]), bmap, [1, 2, 3], 3, home=[0, 1, 0])
    r = check(gpu_ctx, c)
    assert set(r.roof[bmap == 0].ravel()) == {1, 3} and (r.roof[bmap == 1] == 2).all()
    assert (r.roof[bmap == 2] == 0).all() and r.unroofed_pixels == 9  # no seed: stays 0, although 2 lies beside it
    assert (r.height[bmap == 2] == I32_MIN).all()


def test_fill_ring_crosses_every_round_grouping(gpu_ctx):
    n = 300
    bmap = np.full((n, n), -1, np.int32)
    bmap[0, :] = bmap[-1, :] = bmap[:, 0] = bmap[:, -1] = 0
    r = check(gpu_ctx, case(pts([(7, 0)]), bmap, [1], 1))
    assert r.fill_rounds == (4 * n - 4) // 2 >= 150 and r.filled_pixels == 4 * n - 5 and r.unroofed_pixels == 0


# ---- sizes ---------------------------------------------------------------------------------------------------------
def _random_case(h, w, n, n_planes, seed, bin_=7, block=1, cover=1.0):
    rng = np.random.default_rng(seed)
    coarse = rng.random((-(-h // block), -(-w // block))) < 0.3  # (below the percolation threshold: many buildings)
    mask = np.kron(coarse, np.ones((block, block), bool))[:h, :w]
    b = bref.building_map(mask)
    nb = max(b.n_buildings, 1)
    xyz = np.stack([rng.integers(0, max(int(w * bin_ * cover), 1), n), rng.integers(0, h * bin_, n), rng.integers(0, 5000, n)],
                   1).astype(np.int32)
    under = b.map[xyz[:, 1] // bin_, xyz[:, 0] // bin_]
    home = (np.arange(n_planes) % nb).astype(np.int32)
    # a plane at home under the point (building + a multiple of the number of buildings), sometimes any label
    k = rng.integers(0, max(n_planes // nb, 1), n)
    plane = np.where((under >= 0) & (rng.random(n) < 0.8), np.minimum(under + k * nb, n_planes - 1) + 1,
                     rng.integers(-1, n_planes + 2, n)).astype(np.int32)
    normal = rng.normal(size=(n_planes, 3))
    normal[:, 2] = np.abs(normal[:, 2]) + 0.3
    center = np.stack([rng.integers(0, w * bin_, n_planes), rng.integers(0, h * bin_, n_planes), rng.integers(1000, 4000, n_planes)], 1)
    return case(xyz, b.map, plane, n_planes, home, normal, center, bin=bin_, ground_th=800.0, min_votes=1)


@pytest.mark.parametrize("shape", [(1, 1), (16, 64), (15, 63), (17, 65), (1000, 62)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_sizes(gpu_ctx, shape):
    h, w = shape
    for k, n in enumerate((max(h * w // 3, 1), 4 * h * w)):
        c = _random_case(h, w, n, 200, 100 * h + w + k, block=1 if h * w < 100 else 3)
        r = check(gpu_ctx, c)
        assert h * w == 1 or r.seeded_pixels > 0


def test_image_2049_x_2051_with_blobs(gpu_ctx):
    c = _random_case(2049, 2051, 2_000_000, 6000, 3, bin_=5, block=16)
    r = check(gpu_ctx, c)
    assert r.seeded_pixels > 200_000 and r.filled_pixels > 500_000 and r.fill_rounds >= 3 and (r.pixels[2048:] > 0).sum() > 1000


# ---- figures and heights -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_planes", [5000, 70_001], ids=["above_the_lds_tables", "70001_planes"])
@pytest.mark.parametrize("order", ["random", "by_pixel"])
def test_more_planes_than_the_lds_tables(gpu_ctx, n_planes, order):
    """Planes above 2048 take the global-atomic path of both figure passes; 70 001 planes over 300 x 300 pixels need a
    key of 33 bits.  by_pixel: 64 consecutive points in one pixel and plane, so that whole waves reduce in registers."""
    c = _random_case(300, 300, 200_000, n_planes, n_planes, block=6)
    if order == "by_pixel":
        o = np.argsort((c["xyz"][:, 1] // 7) * 300 + c["xyz"][:, 0] // 7, kind="stable")[::64]
        c["xyz"] = np.ascontiguousarray(np.repeat(c["xyz"][o], 64, axis=0))
        c["xyz"][:, 2] = 1000 + (np.arange(len(c["xyz"])) % 64).astype(np.int32) * 13  # (all above the ground threshold)
        c["plane_idx"] = np.ascontiguousarray(np.repeat(c["plane_idx"][o], 64))
    r = check(gpu_ctx, c)
    assert (r.n_support[2048:] > 0).sum() > 50 and (r.n_support[:2048] > 0).any() and (r.pixels[2048:] > 0).sum() > 50
    if n_planes > 70_000:
        assert (r.pixels[65_536:] > 0).any() and 300 * 300 * n_planes >= 2 ** 32
    if order == "by_pixel":
        assert (r.n_support % 64 == 0).all()


def test_heights_flat_steep_and_degenerate_planes(gpu_ctx):
    bmap = np.repeat(np.arange(6, dtype=np.int32), 20).reshape(6, 20)  # six buildings, one row each
    nan = float("nan")
    normal = [[0, 0, 1.0], [0.3, 0.0, 0.9], [0.3, 0.1, 0.0], [0.3, 0.0, -0.5], [nan, 0.0, 1.0], [0.2, 0.1, 0.9]]
    center = [[1000, 50, 3210], [1000, 150, 3000], [1000, 250, 3000], [1000, 350, 3000], [1000, 450, 3000], [1000, 550, 3000]]
    px = [(x, y) for y in range(6) for x in (2, 17)]
    xyz = pts(px, bin=100)
    xyz[:, 2] = [2900, 3100] * 6
    c = case(xyz, bmap, np.repeat(np.arange(1, 7), 2), 6, home=np.arange(6), normal=normal, center=center, bin=100)
    r = check(gpu_ctx, c)
    assert (r.z_min == 2900).all() and (r.z_max == 3100).all()
    assert (r.height[0] == 3100).all()  # flat: cz = 3210, above every supporting point: the upper clamp
    c["center"][0, 2] = 3050
    r = check(gpu_ctx, c)
    assert (r.height[0] == 3050).all()  # flat and inside the clamps: H == cz
    assert r.height[1, 0] == 3100 and r.height[1, -1] == 2900 and len(set(r.height[1].tolist())) > 2  # steep: both clamps
    assert set(r.height[2].tolist()) <= {2900, 3100}  # nz == 0: +-inf, clamped (and NaN at t == 0: z_min)
    assert r.height[3, 0] < r.height[3, -1]  # nz < 0 is not an error: the slope just turns round
    assert (r.height[4] == 2900).all()  # NaN: z_min
    assert (r.height[5] == rr.height_of(np.full(20, 6), np.arange(20) * 100 + 50, np.full(20, 550), c["normal"], c["center"],
                                        r.z_min, r.z_max)).all()


def test_optional_outputs_and_device_pointers(gpu_ctx):
    import torch
    c = fz.fuzz_case(17)
    want = fz.run_ref(c)
    for sup, hgt in ((False, True), (True, False), (False, False)):
        r = run(gpu_ctx, c, support=sup, height=hgt)
        same(r, want, images=("roof",) + (("support",) if sup else ()) + (("height",) if hgt else ()))
        assert (r.support is None) == (not sup) and (r.height is None) == (not hgt)
        assert (r.info["ms_height"] > 0) == hgt and r.info["ms_vote"] > 0 and r.info["ms_fill"] > 0 and r.info["ms_figures"] > 0
    h, w = c["bmap"].shape
    d_xyz, d_map, d_pl = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("xyz", "bmap", "plane_idx"))
    for sup, hgt in ((True, True), (False, True), (True, False), (False, False)):
        d_roof, d_sup, d_hgt = (torch.full((h, w), -77, dtype=torch.int32, device="cuda") for _ in range(3))
        r = gpu_ctx.roofs_dev(d_xyz.data_ptr(), len(c["xyz"]), d_map.data_ptr(), w, h, d_pl.data_ptr(), c["home"], c["normal"],
                              c["center"], d_roof.data_ptr(), d_sup.data_ptr() if sup else 0, d_hgt.data_ptr() if hgt else 0,
                              bin=c["bin"], ground_th=c["ground_th"], min_votes=c["min_votes"])
        same_figures(r, want)
        assert np.array_equal(d_roof.cpu().numpy(), want.roof)
        assert np.array_equal(d_sup.cpu().numpy(), want.support) if sup else (d_sup == -77).all().item()
        assert np.array_equal(d_hgt.cpu().numpy(), want.height) if hgt else (d_hgt == -77).all().item()


def test_no_planes_at_all(gpu_ctx):
    bmap = np.array([[0, -1, 1], [0, 0, 1]], np.int32)
    c = case(pts([(0, 0), (2, 1)]), bmap, [1, -1], 0)
    r = check(gpu_ctx, c)
    assert r.roof.tolist() == [[0, -1, 0], [0, 0, 0]] and r.unroofed_pixels == 5 and r.pixels.shape == (0,)
    L, out = gpu_ctx._L, _lib.Roofs()
    roof = np.empty((2, 3), np.int32)
    rc = L.bs_roofs(gpu_ctx._h, c["xyz"].ctypes.data, 2, 10, 0.0, bmap.ctypes.data, 3, 2, c["plane_idx"].ctypes.data, 0, None,
                    None, None, 1, roof.ctypes.data, None, None, C.byref(out))  # the tables are not read
    assert rc == 0 and roof.tolist() == r.roof.tolist() and out.n_planes == 0
    L.bs_roofs_free(C.byref(out))


# ---- errors --------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_and_the_context_alone(gpu_ctx):
    import torch
    c = fz.fuzz_case(13)
    want = fz.run_ref(c)
    h, w = c["bmap"].shape
    n, bin_ = len(c["xyz"]), c["bin"]

    def raises(status, fn, *a, **kw):
        with pytest.raises(api.BsError) as e:
            fn(*a, **kw)
        assert e.value.status == status

    d_map, d_pl = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("bmap", "plane_idx"))
    outs = [torch.full((h, w), -77, dtype=torch.int32, device="cuda") for _ in range(3)]
    tabs = (c["home"], c["normal"], c["center"])

    def dev(d_xyz, **kw):
        a = dict(n=n, d_map=d_map.data_ptr(), w=w, h=h, d_pl=d_pl.data_ptr(), d_roof=outs[0].data_ptr(), bin=bin_, min_votes=1,
                 n_planes=None)
        a.update(kw)
        return gpu_ctx.roofs_dev(d_xyz, a["n"], a["d_map"], a["w"], a["h"], a["d_pl"], *tabs, a["d_roof"], outs[1].data_ptr(),
                                 outs[2].data_ptr(), bin=a["bin"], ground_th=c["ground_th"], min_votes=a["min_votes"],
                                 n_planes=a["n_planes"])

    for bad in ([w * bin_, 5, 0], [5, h * bin_, 0], [-1, 5, 0], [5, -1, 0]):  # a pixel outside the image
        p = c["xyz"].copy()
        p[n // 2] = bad
        raises(-2, run, gpu_ctx, dict(c, xyz=p))
        raises(-2, dev, torch.from_numpy(p).cuda().data_ptr())
        assert all((o == -77).all().item() for o in outs)  # the outputs are left untouched
    d_xyz = torch.from_numpy(c["xyz"]).cuda()
    x = d_xyz.data_ptr()
    raises(-2, dev, x, n=2 ** 29)
    for kw in (dict(n=0), dict(bin=0), dict(w=0), dict(h=0), dict(n_planes=-1), dict(min_votes=0), dict(d_map=0), dict(d_pl=0),
               dict(d_roof=0)):
        raises(-1, dev, x, **kw)
    raises(-1, dev, 0)
    raises(-1, run, gpu_ctx, dict(c, min_votes=0))
    raises(-1, run, gpu_ctx, dict(c, bin=0))
    L, out = gpu_ctx._L, _lib.Roofs()
    nrm, ctr, hm = (np.ascontiguousarray(t) for t in (c["normal"], c["center"], c["home"]))
    for t in ((None, nrm.ctypes.data, ctr.ctypes.data), (hm.ctypes.data, None, ctr.ctypes.data), (hm.ctypes.data, nrm.ctypes.data, None)):
        assert L.bs_roofs_dev(gpu_ctx._h, x, n, bin_, 0.0, d_map.data_ptr(), w, h, d_pl.data_ptr(), c["n_planes"], *t, 1,
                              outs[0].data_ptr(), None, None, C.byref(out)) == -1
    assert L.bs_roofs_dev(gpu_ctx._h, x, n, bin_, 0.0, d_map.data_ptr(), w, h, d_pl.data_ptr(), c["n_planes"], hm.ctypes.data,
                          nrm.ctypes.data, ctr.ctypes.data, 1, outs[0].data_ptr(), None, None, None) == -1
    assert b"roofs" in L.bs_last_error(gpu_ctx._h)
    assert all((o == -77).all().item() for o in outs)
    same(run(gpu_ctx, c), want)  # and the context still works
    dev(x, min_votes=c["min_votes"])
    assert np.array_equal(outs[0].cpu().numpy(), want.roof) and np.array_equal(outs[2].cpu().numpy(), want.height)


# ---- fuzz ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(fz.N_CASES))
def test_fuzz_against_the_restatement(gpu_ctx, seed):
    c = fz.fuzz_case(seed)
    r = check(gpu_ctx, c)
    again = run(gpu_ctx, c)
    same(again, r)  # and two runs give identical arrays


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_gabled_scene_end_to_end(gpu_ctx, tmp_path):
    sc = load_roof_scenes()
    xyz = sc.gabled()
    _, _, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=15))
    n_planes = len(planes)
    fp, b, r = gpu_ctx.roof_model(xyz, plane_idx, planes)
    _, b0 = gpu_ctx.buildings(xyz, plane_idx, n_planes)
    assert np.array_equal(b.map, b0.map) and np.array_equal(b.votes.plane_building, b0.votes.plane_building)
    normal, center = np.array([p.normal for p in planes]), np.array([p.center for p in planes], np.int32)
    home = rr.homes(normal, b.votes.plane_building, b.votes.votes_in, b.votes.votes_total)
    assert np.array_equal(r.home, home) and np.array_equal(r.normal, normal) and np.array_equal(r.center, center)
    want = rr.roofs(xyz, b.map, plane_idx, n_planes, home, normal, center, 100, b.ground_th, 1)
    same(r, want)
    check_gabled_facts(sc, b.map, b.n_buildings, home, normal, center, plane_idx, n_planes, r)
    origin = (431200, 5620000, 87000)
    api.write_roofs_obj(r, b.map, tmp_path / "roofs.obj", origin=origin)
    assert (tmp_path / "roofs.obj").read_bytes() == rr.obj_text(want.roof, b.map, want.pixels, want.z_min, want.z_max, normal,
                                                                 center, 100, origin)
