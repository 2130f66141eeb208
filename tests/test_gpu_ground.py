"""The ground stage on the device (bs_ground, bs_ground_dev; include/bs_api.h) against the numpy restatement
tests/ground_ref, and the ground model (bs_set_ground_model) in the raster, the point assignment and the roofs against
their references run with the per-point rule.  Everything is an exact integer: every comparison is ==."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_ground_cpu import BY_NAME, EMPTY, HERE, brute, cases, gref, ref  # noqa: E402

sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
sys.path.insert(0, os.path.join(HERE, "building_ref"))
sys.path.insert(0, os.path.join(HERE, "roof_ref"))
import building_ref as bref  # noqa: E402
import ref as fref  # noqa: E402
import roof_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
PATTERN = -0x5A5A5A5B
ARRAYS = ("low", "dtm", "step", "hag", "cls")
SCALARS = ("width", "height", "threshold", "step_pixels") + gref.FIGURES
_BIG = []


def run(ctx, c, **kw):
    return ctx.ground(c["xyz"], c["extent"], c["params"], **kw)


def differs(got, want, arrays=ARRAYS):
    """None if the device's Ground equals the restatement's result everywhere, else the first name that differs"""
    for k in SCALARS:
        if getattr(got, k) != getattr(want, k):
            return k, getattr(got, k), getattr(want, k)
    for k in arrays:
        a, b = getattr(got, k), getattr(want, k)
        if a.dtype != b.dtype or not np.array_equal(a, b):
            return k
    return None


def big():
    if not _BIG:
        c = cases.big()
        _BIG.extend([c, gref.ground(*cases.args(c))])
    return _BIG


def on_device(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("name", [c["name"] for c in cases.CASES])
def test_case(gpu_ctx, name):
    """every case through the host entry point: low, dtm, step, hag, class and every figure"""
    got, want = run(gpu_ctx, BY_NAME[name]), ref(name)
    assert differs(got, want) is None, (name, differs(got, want))
    assert got.cell == BY_NAME[name]["params"]["cell"] and got.radius == BY_NAME[name]["params"]["radius"]
    assert got.n_points == len(BY_NAME[name]["xyz"]) and (got.grid, got.row_lds) == (_lib.GROUND_GRID, _lib.GROUND_ROW_LDS)


def test_cases_on_the_device(gpu_ctx):
    """what the cases are for, read from the device's result"""
    a = run(gpu_ctx, BY_NAME["hole"])
    x0, y0, x1, y1 = cases.HOLE
    assert a.n_filled_pixels > 0 < a.n_empty_pixels - a.n_filled_pixels
    assert a.dtm[(y0 + y1) // 2, (x0 + x1) // 2] == EMPTY and a.dtm[y0, x0] != EMPTY
    a = run(gpu_ctx, BY_NAME["edge_equal"])
    (xe, ye), (xo, yo) = cases.EDGE_EQUAL, cases.EDGE_OVER
    assert a.step[ye, xe] == 0 and a.step[yo, xo] == 1 and a.step_pixels == [9]
    a = run(gpu_ctx, BY_NAME["first_flag"])
    assert a.step[cases.SPIKE[1], cases.SPIKE[0]] == 1 and a.step_pixels == [1, 24]
    a = run(gpu_ctx, BY_NAME["cap"])
    assert a.threshold == [230, 230, 260, 300] and a.step_pixels == [0, 0, 0, 144]
    a = run(gpu_ctx, BY_NAME["negative"])
    assert a.dtm_min == -cases.Z_LIMIT and a.low.max() == cases.Z_LIMIT
    a = run(gpu_ctx, BY_NAME["slope_200"])
    print("slope_200:", a.step_pixels, a.n_ground_points, a.n_low_points, a.n_object_points, a.info)


def test_a_second_point_per_thread(gpu_ctx):
    """more points than one sweep of the two passes over the points (BS_GROUND_GRID workgroups of 256): some threads take
    a second point, their figures kept"""
    c, want = big()
    got = run(gpu_ctx, c)
    assert differs(got, want) is None, differs(got, want)
    assert got.grid * 256 < got.n_points < 2 * got.grid * 256
    figures_only = run(gpu_ctx, c, images=False, points=False)
    assert figures_only.dtm is None and figures_only.hag is None and differs(figures_only, want, ()) is None


def test_null_outputs_and_errors(gpu_ctx):
    """the device entry point: each output NULL in turn, and every error of the definition: the outputs and the struct are
    untouched, and the context stays usable"""
    import torch
    ctx = gpu_ctx
    c = BY_NAME["odd"]
    want = ref("odd")
    w, h, n = want.width, want.height, len(c["xyz"])
    d_xyz, = on_device(c["xyz"])
    shapes = (((h, w), torch.int32, PATTERN), ((h, w), torch.int32, PATTERN), ((h, w), torch.uint8, 0xA5), ((n,), torch.int32, PATTERN),
              ((n,), torch.uint8, 0xA5))
    outs = [torch.full(s, f, dtype=dt, device="cuda") for s, dt, f in shapes]
    fills = [f for _, _, f in shapes]
    ptrs = [o.data_ptr() for o in outs]
    ext = np.ascontiguousarray(c["extent"], np.int32)

    def stage(out, xyz=d_xyz.data_ptr(), n=n, extent=ext, params=c["params"], outputs=ptrs):
        q = C.byref(api._ground_struct(params)) if params is not None else None
        return ctx._L.bs_ground_dev(ctx._h, xyz, n, extent.ctypes.data if extent is not None else None, q, *outputs, out)

    def untouched(**kw):
        out = _lib.Ground()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        rc = stage(C.byref(out), **kw)
        msg = ctx._L.bs_last_error(ctx._h)
        torch.cuda.synchronize()
        assert bytes(out) == b"\x5a" * C.sizeof(out) and all(bool((o == f).all()) for o, f in zip(outs, fills)), kw
        return rc, msg

    def moved(col, v):
        x = c["xyz"].copy()
        x[n // 2, col] = v
        return on_device(x)[0]

    p = c["params"]
    assert stage(None) == -1
    invalid = [dict(xyz=None), dict(extent=None), dict(params=None), dict(n=0), dict(extent=np.array([-1, 5, 0], np.int32))]
    invalid += [dict(params=dict(p, **kw)) for kw in (dict(cell=0), dict(radius=[]), dict(radius=[0]), dict(radius=[256]),
                                                      dict(radius=[2, 2]), dict(radius=[3, 2]), dict(s_num=-1), dict(s_den=0),
                                                      dict(dh0=-1), dict(dh_max=-1), dict(tol=-1), dict(min_height=-1))]
    for kw in invalid:
        assert untouched(**kw)[0] == -1, kw
    q = api._ground_struct(p)
    q.n_steps = 17
    out = _lib.Ground()
    assert ctx._L.bs_ground_dev(ctx._h, d_xyz.data_ptr(), n, ext.ctypes.data, C.byref(q), *ptrs, C.byref(out)) == -1
    rc, msg = untouched(n=1 << 29)
    assert rc == -2 and b"2^29" in msg
    rc, msg = untouched(extent=np.array([2 ** 31 - 1, 2 ** 31 - 1, 0], np.int32), params=dict(p, cell=1))
    assert rc == -2 and b"pixels" in msg
    for col, v, word in ((0, -1, b"negative"), (1, -1, b"negative"), (0, w * p["cell"], b"outside"), (1, h * p["cell"], b"outside"),
                         (2, 1 << 23, b"2^23"), (2, -(1 << 23), b"2^23")):
        bad = moved(col, v)
        rc, msg = untouched(xyz=bad.data_ptr())
        assert rc == -2 and word in msg, (col, v, msg)
    # each output NULL in turn, and all of them: the outputs given are written
    names = ("d_low", "d_dtm", "d_step", "d_hag", "d_class")
    for skip in (0, 1, 2, 3, 4, (0, 1, 2, 3, 4)):
        skip = (skip,) if isinstance(skip, int) else skip
        for o, f in zip(outs, fills):
            o.fill_(f)
        got = ctx.ground_dev(d_xyz.data_ptr(), n, ext, p, **{k: (0 if j in skip else q) for j, (k, q) in enumerate(zip(names, ptrs))})
        assert got.dtm is None and differs(got, want, ()) is None, differs(got, want, ())
        for j, (o, f, field) in enumerate(zip(outs, fills, ARRAYS)):
            a = o.cpu().numpy()
            assert np.array_equal(a, np.full(a.shape, f, a.dtype) if j in skip else getattr(want, field)), (skip, field)
    with pytest.raises(api.BsError):
        ctx.ground(c["xyz"], c["extent"], dict(p, radius=[4, 2]))
    out = _lib.Ground()
    ctx._L.bs_ground_free(C.byref(out))  # a zeroed struct
    ctx._L.bs_ground_free(None)
    assert differs(run(ctx, c), want) is None  # the context stays usable


# ---- the switch: the ground model in the raster, the assignment and the roofs -------------------------------------------------
BIN = 100


def labelled_scene(rise):
    """the dense scene with plane labels by construction: plane c + 1 the roof of box c, plane 4 the ground, 0 the walls"""
    xyz = cases.scene(rise)
    x, y, z = (xyz[:, k].astype(np.int64) for k in range(3))
    plane = np.zeros(len(xyz), np.int32)
    for c, (x0, x1, y0, y1) in enumerate(cases.SLOPE_BOXES):  # (the scene's shift to its origin is inside the margins)
        top = (x0 + x1) // 2 * rise // 1000 + cases.SLOPE_HEIGHT
        inside = (x >= x0 - 60) & (x <= x1 + 20) & (y >= y0 - 60) & (y <= y1 + 20)
        plane[inside & (np.abs(z - top) <= 30)] = c + 1
    plane[(plane == 0) & (np.abs(z - x * rise // 1000) <= 40)] = 4
    return xyz, plane


def model_of(rise, cell=500):
    xyz = cases.scene(rise)
    p = gref.params(cell=cell)
    return gref.ground(xyz, xyz.max(0), p), p


def ref_map(xyz, th, model):
    """(mask of the kept points, closed mask, building map of tests/building_ref) under the rule"""
    m = gref.splat_mask(xyz, ~gref.below(xyz, th, model), xyz.max(0), BIN)
    _, closed = fref.footprints(fref.image_of_mask(m))
    return m, closed, bref.building_map(closed)


def raster_bytes(ctx, xyz):
    img, th = ctx.grid_picture(xyz, bin=BIN)
    return img.tobytes(), th


def consumers(ctx, xyz, plane, bmap, nb, home, th):
    """the three consumers under whatever model the context holds: (image, ground_th, building_idx, figures, Roofs)"""
    img, th2 = ctx.grid_picture(xyz, bin=BIN)
    assert th2 == th
    _, b = ctx.building_map(bmap >= 0)
    assert b.n_buildings == nb
    bidx = ctx.assign_buildings(xyz, bmap, b, bin=BIN, ground_th=th)
    normal = np.tile([0.0, 0.0, 1.0], (4, 1))
    center = np.tile(np.array([0, 0, 4000], np.int32), (4, 1))
    r = ctx.roofs(xyz, bmap, plane, home, normal, center, bin=BIN, ground_th=th)
    return img, bidx, b, r


def check_consumers(got, xyz, plane, bmap, nb, home, th, model):
    """the device's three results against their references run with the per-point rule"""
    img, bidx, b, r = got
    keep = ~gref.below(xyz, th, model)
    # the raster: the mask of its density channel is the pixels a kept point touches
    assert np.array_equal(fref.mask(img), gref.splat_mask(xyz, keep, xyz.max(0), BIN))
    # the assignment: every point's building, n_points over all points, the other figures over the kept points alone
    every = bref.assign(xyz, bmap, nb, BIN, np.inf)
    kept = bref.assign(xyz[keep], bmap, nb, BIN, -np.inf)
    assert np.array_equal(bidx, every.building_idx) and np.array_equal(b.n_points, every.n_points)
    for k in ("n_above", "z_min", "z_max", "z_sum"):
        assert np.array_equal(getattr(b, k), getattr(kept, k)), k
    # the roofs: the points that fail the rule carry no plane
    normal = np.tile([0.0, 0.0, 1.0], (4, 1))
    center = np.tile(np.array([0, 0, 4000], np.int32), (4, 1))
    want = rr.roofs(xyz, bmap, np.where(keep, plane, 0), 4, home, normal, center, bin=BIN, ground_th=-np.inf)
    for k in ("roof", "support", "height"):
        assert np.array_equal(getattr(r, k), getattr(want, k)), k
    for k in rr.FIGURES:
        assert np.array_equal(getattr(r, k), getattr(want, k)), k
    for k in rr.TOTALS:
        assert getattr(r, k) == getattr(want, k), k
    return keep


def consumer_bytes(got):
    img, bidx, b, r = got
    parts = [img, bidx] + [getattr(b, k) for k in ("n_points", "n_above", "z_min", "z_max", "z_sum")]
    parts += [r.roof, r.support, r.height] + [getattr(r, k) for k in rr.FIGURES]
    return b"".join(np.ascontiguousarray(a).tobytes() for a in parts) + repr([getattr(r, k) for k in rr.TOTALS]).encode()


def test_switch_on_the_three_consumers(gpu_ctx):
    """with the model set, the raster's mask, the assignment and the roofs equal their references run with the per-point
    rule; a table that ends inside the cloud, or holds EMPTY, leaves the points beyond it to the scalar rule; switched off
    again every byte is that of a run before the switch was ever set; a batch of two tiles refuses while it is on"""
    ctx = gpu_ctx
    rise = 100
    xyz, plane = labelled_scene(rise)
    assert all((plane == k).sum() > 1000 for k in range(5))
    g, p = model_of(rise)
    th = gref.ground_th(xyz)
    full = (g.dtm, p["cell"], p["min_height"])
    _, _, bm = ref_map(xyz, th, full)
    bmap, nb = bm.map, bm.n_buildings
    assert nb == 3
    home = np.array([bmap[(y0 + y1) // 2 // BIN, (x0 + x1) // 2 // BIN] for x0, x1, y0, y1 in cases.SLOPE_BOXES] + [0], np.int32)
    assert sorted(home[:3].tolist()) == [0, 1, 2] and ctx.ground_model() is None
    before = consumers(ctx, xyz, plane, bmap, nb, home, th)
    scalar_keep = check_consumers(before, xyz, plane, bmap, nb, home, th, None)
    # the whole table
    ctx.set_ground_model(g.dtm, p["cell"], p["min_height"])
    t, cell, mh = ctx.ground_model()
    assert np.array_equal(t, g.dtm) and (cell, mh) == (p["cell"], p["min_height"])
    on = consumers(ctx, xyz, plane, bmap, nb, home, th)
    keep = check_consumers(on, xyz, plane, bmap, nb, home, th, full)
    assert (keep != scalar_keep).sum() > 1000 and consumer_bytes(on) != consumer_bytes(before)
    # a batch of two tiles refuses; a batch of one works and is the solo raster
    with pytest.raises(api.BsError, match="more than one tile"):
        ctx.grid_picture_batch([xyz, xyz], bin=BIN)
    one = ctx.grid_picture_batch([xyz], bin=BIN)
    assert np.array_equal(one[0][0], on[0])
    # a table that ends in the middle of the cloud and has EMPTY pixels: those points fall back to the scalar rule
    part = g.dtm[:, :g.width // 2].copy()
    part[::3, ::4] = EMPTY
    ctx.set_ground_model(part, p["cell"], p["min_height"])
    half = consumers(ctx, xyz, plane, bmap, nb, home, th)
    keep_half = check_consumers(half, xyz, plane, bmap, nb, home, th, (part, p["cell"], p["min_height"]))
    outside = xyz[:, 0] // p["cell"] >= part.shape[1]
    assert outside.sum() > 1000 and np.array_equal(keep_half[outside], scalar_keep[outside])
    assert (keep_half[~outside] != scalar_keep[~outside]).any() and (keep_half != keep).any()
    # from a device table
    d_dtm, = on_device(g.dtm)
    ctx.set_ground_model((d_dtm.data_ptr(), g.width, g.height), p["cell"], p["min_height"], device=True)
    assert np.array_equal(ctx.ground_model()[0], g.dtm)
    assert consumer_bytes(consumers(ctx, xyz, plane, bmap, nb, home, th)) == consumer_bytes(on)
    # off again
    ctx.set_ground_model(None)
    assert ctx.ground_model() is None
    assert consumer_bytes(consumers(ctx, xyz, plane, bmap, nb, home, th)) == consumer_bytes(before)
    two = ctx.grid_picture_batch([xyz, xyz], bin=BIN)
    assert np.array_equal(two[1][0], before[0])
    for kw in (dict(cell=0), dict(min_height=-1)):
        with pytest.raises(api.BsError):
            ctx.set_ground_model(g.dtm, **dict(dict(cell=500, min_height=2000), **kw))
    assert ctx.ground_model() is None


# ---- end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rise", [100, 200])
def test_end_to_end_buildings(gpu_ctx, rise):
    """Context.buildings(ground={}) finds the three boxes on the slope, its map is the restatement's; ground=None gives
    the scalar map, which loses them"""
    ctx = gpu_ctx
    xyz = cases.scene(rise)
    truth = cases.slope_map(BIN)
    out = ctx.buildings(xyz, bin=BIN, ground={})
    assert len(out) == 3 and ctx.ground_model() is None  # the previous switch is restored
    fp, b, g = out
    want_g, p = model_of(rise)
    assert differs(g, want_g, ("low", "dtm", "step")) is None and g.hag is None
    th = gref.ground_th(xyz)
    _, _, want = ref_map(xyz, th, (want_g.dtm, p["cell"], p["min_height"]))
    scores = gref.box_scores(b.map, truth)
    print(f"model, rise {rise}: buildings {b.n_buildings}, IoU {scores}")
    assert b.n_buildings == 3 and np.array_equal(b.map, want.map) and b.ground_th == th and min(scores) >= 0.99
    fp0, b0 = ctx.buildings(xyz, bin=BIN)
    _, _, want0 = ref_map(xyz, th, None)
    scores0 = gref.box_scores(b0.map, truth)
    print(f"scalar rule, rise {rise}: ground_th {th}, buildings {b0.n_buildings}, IoU {scores0}")
    assert np.array_equal(b0.map, want0.map)
    if rise == 100:
        assert min(scores0) < 0.5
    else:
        assert b0.n_buildings < 3
    # a model of the context's own survives the call
    ctx.set_ground_model(want_g.dtm[:4, :4], 500, 7)
    try:
        assert np.array_equal(ctx.buildings(xyz, bin=BIN, ground={})[1].map, b.map)
        t, cell, mh = ctx.ground_model()
        assert np.array_equal(t, want_g.dtm[:4, :4]) and (cell, mh) == (500, 7)
    finally:
        ctx.set_ground_model(None)


def test_end_to_end_solids(gpu_ctx):
    """segment -> solid_model(ground={}, terrain={}) on the 20 % slope: three buildings, each a closed solid that stands on
    its own ground"""
    from test_solids_cpu import load_solid_cases
    sr = load_solid_cases().sr
    ctx = gpu_ctx
    xyz = cases.scene(200)
    _, _, plane_idx, planes = ctx.segment(xyz, api.default_params(k=15))
    out = ctx.solid_model(xyz, plane_idx, planes, refit=True, ground={}, terrain={})
    assert len(out) == 6 and ctx.ground_model() is None and ctx.building_bases() is None
    fp, b, roofs, s, t, g = out
    print("slope_200 solids:", b.n_buildings, t.ground.tolist(), s.pixels.tolist(), s.volume6.tolist())
    assert b.n_buildings == 3 and s.n_buildings == 3 and (s.pixels > 0).all() and t.n_fallback == 0
    assert sr.unmatched_edges(s) == 0 and np.array_equal(s.base, t.ground)
    assert (np.diff(np.sort(t.ground)) > 2000).all()  # 17 m apart on 20 %
    scores = gref.box_scores(b.map, cases.slope_map(BIN))
    assert min(scores) >= 0.99
    out3 = ctx.roof_model(xyz, plane_idx, planes, refit=True, ground={})
    assert len(out3) == 4 and np.array_equal(out3[1].map, b.map) and np.array_equal(out3[2].roof, roofs.roof)
    assert len(ctx.solid_model(xyz, plane_idx, planes, refit=True)) == 4  # ground=None returns what it returned before
