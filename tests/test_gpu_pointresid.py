"""Point residuals on the device (bs_point_residuals, bs_point_residuals_dev; include/bs_api.h) against the numpy restatement
tests/pointresid_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_pointresid_cpu import BY_NAME, NB_LABEL, NB_NAME, NB_TOL, cases, cloud, ref, upstream  # noqa: E402

pref, brute, mref, tref = cases.pref, cases.brute, cases.mref, cases.mc.tref

pytestmark = pytest.mark.gpu
PATTERN = -0x5A5A5A5B
# the runs of the device suite: the shapes of the threshold table ("Point residuals") and two of the imported fuzz
FIGURES = [k for k in pref.DEVICE_FIELDS if k not in brute.ARRAYS]  # (without the per-point arrays)
NAMES = ["bay", "staircase", "band", "wide", "nested", NB_NAME, "fuzz_1", "slope_wide", "slope_narrow"] + \
        [f"pstrip_{n}" for n in cases.STRIPS]


def check(ctx, name, tol, n_random=None):
    """the host-memory entry point against the restatement over the restated stages before: the three per-point arrays and
    every figure"""
    c = BY_NAME[name][0]
    k = cloud(name, tol, n_random)
    want = ref(name, tol, n_random)[0]
    _, clean, tri = upstream(name, tol)
    got, gt, gc, _, _ = ctx.point_residuals(c["label"], c["top"], k.xyz, n_labels=c["n_labels"], num=tol[0], den=tol[1], bin=k.bin,
                                            plane_idx=k.plane_idx, label_plane=k.label_plane, clip2=k.clip2)
    assert pref.same(got, want) is None, (name, tol, pref.same(got, want))
    assert (got.fig_cap, got.chunk, got.grid) == (pref.FIG_CAP, pref.CHUNK, pref.GRID)
    assert tref.same(gt, tri) is None and np.array_equal(gc.sxy, clean.sxy) and np.array_equal(gc.sz, clean.sz)
    return got


def on_device(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


@pytest.mark.parametrize("name", sorted(set(NAMES)))
def test_case(gpu_ctx, name):
    """every named run at every tolerance of its own"""
    for tol in BY_NAME[name][1]:
        check(gpu_ctx, name, tol)


def test_shapes_on_the_device(gpu_ctx):
    """what the shapes are for, read from the device's result"""
    s = check(gpu_ctx, "staircase", (1, 1))
    trace = ref("staircase", (1, 1))[1]
    assert trace["tie_owned"] > 0 and trace["tie_not_owned"] > 0 and s.n_multi == 0  # a centre on a slanted edge: both outcomes
    b = check(gpu_ctx, "bay", (100, 1))
    assert b.n_multi > 0 and b.multi[1] == 0 and (b.cover > 1).any() and b.n_uncovered > 0  # twice: the lowest slot, label 0's
    f = check(gpu_ctx, NB_NAME, NB_TOL)
    assert f.points[NB_LABEL] == 0 and not (f.label == NB_LABEL).any() and f.n_uncovered > 0
    d = check(gpu_ctx, "band", (2, 1))
    assert d.max_list > 1 and d.n_empty_pixel > 0 and d.n_rows > 1000
    assert ref("wide", (0, 1))[1]["max_span"] > check(gpu_ctx, "wide", (0, 1)).chunk
    for n in cases.STRIPS:
        p = check(gpu_ctx, f"pstrip_{n}", (0, 1))
        assert len(p.points) == n and (p.points >= 1).all()
    w, nar = check(gpu_ctx, "slope_wide", (0, 1)), check(gpu_ctx, "slope_narrow", (0, 1))
    assert w.n_height_wide == w.total_points == w.n_points > 0  # the height beyond 64 bits
    assert nar.n_height_wide == 0 and nar.total_points == nar.n_points > 0  # and the run that stays in them
    print("band:", d.n_rows, d.n_items, d.max_list, d.n_empty_pixel, "slope:", w.max_abs_r2_all, w.info)


def test_a_second_point_per_thread(gpu_ctx):
    """more points than one sweep of the pass over the points (BS_PRESID_GRID workgroups of 256): some threads take a second
    point with their register totals and LDS tables kept"""
    r = check(gpu_ctx, "nested", (2, 1), n_random=600_000)
    assert r.grid * 256 < r.n_points < 2 * r.grid * 256 and r.total_points > r.grid * 128


@pytest.mark.parametrize("name,tol", [("nested", (2, 1)), ("bay", (100, 1))])
def test_bin_1_equals_the_model_raster(gpu_ctx, name, tol):
    """one point per pixel in raster order at bin 1 against bs_model_raster_dev on the same state: M, cover and mz2 (nested:
    every pixel covered once; the bay: pixels covered twice and not at all)"""
    import torch
    ctx = gpu_ctx
    c = BY_NAME[name][0]
    h, w = c["label"].shape
    xyz = cases.raster_cloud(c)
    d_label, d_top, d_xyz = on_device(c["label"], c["top"], xyz)
    ctx.outline_triangles_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, c["n_labels"], *tol)
    imgs = [torch.full((h, w), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3)]
    ctx.model_raster_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, *[i.data_ptr() for i in imgs])
    outs = [torch.full((h * w,), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3)]
    r = ctx.point_residuals_dev(d_xyz.data_ptr(), h * w, 1, d_label_out=outs[0].data_ptr(), d_r2=outs[1].data_ptr(),
                                d_cover=outs[2].data_ptr())
    model, cover, mz2 = (i.cpu().numpy().reshape(-1) for i in imgs)
    label, r2, cov = (o.cpu().numpy() for o in outs)
    assert np.array_equal(label, model) and np.array_equal(cov, cover) and (model >= 0).any()
    assert (name == "nested") == bool((cover == 1).all())
    assert np.array_equal(np.where(label >= 0, 2 * xyz[:, 2].astype(np.int64) - r2, brute.INT32_MIN), mz2)
    assert r.n_points == h * w and r.total_plane_points == 0 and r.total_above == r.total_below == 0


def test_reads_the_state_and_leaves_it(gpu_ctx):
    """poly_solids_dev, then point_residuals_dev, then both emits: byte-identical to a run without the stage in between, and
    the stage equals the host-memory entry point"""
    import torch
    ctx = gpu_ctx
    name, tol = "nested", (2, 1)
    c, _, b = BY_NAME[name]
    k = cloud(name, tol)
    h, w = c["label"].shape
    nl = c["n_labels"]
    lb = (np.arange(nl) % 3).astype(np.int32)
    d_label, d_top, d_lb, d_xyz, d_plane = on_device(c["label"], c["top"], lb, k.xyz, k.plane_idx)

    def mesh(stage):
        s = ctx.poly_solids_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, nl, d_lb.data_ptr(), 3, *tol, bin=b, base_z=-1000)[0]
        bufs = [torch.full(shape, PATTERN if dt != torch.uint8 else 0xA5, dtype=dt, device="cuda")
                for shape, dt in (((s.n_vertices, 4), torch.int32), ((s.n_faces + 1,), torch.int32), ((s.n_indices,), torch.int32),
                                  ((s.n_faces,), torch.int32), ((s.n_faces,), torch.uint8))]
        outs = [torch.full((len(k.xyz),), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3)]
        r = ctx.point_residuals_dev(d_xyz.data_ptr(), len(k.xyz), b, d_plane.data_ptr(), k.label_plane, k.clip2,
                                    *[o.data_ptr() for o in outs]) if stage else None
        ctx.poly_solids_emit_dev(*[x.data_ptr() for x in bufs])
        d_tri = torch.zeros((upstream(name, tol)[2].n_triangles, 3), dtype=torch.int32, device="cuda")
        ctx.outline_triangles_emit_dev(d_tri.data_ptr())
        return b"".join(x.cpu().numpy().tobytes() for x in bufs + [d_tri]), r, [o.cpu().numpy() for o in outs]

    plain, _, _ = mesh(False)
    with_stage, r, outs = mesh(True)
    assert plain == with_stage
    r.label, r.r2, r.cover = outs
    assert pref.same(r, ref(name, tol)[0]) is None, pref.same(r, ref(name, tol)[0])


def test_null_outputs_and_errors(gpu_ctx):
    """each output NULL in turn, no plane table, clip2 = 0, and every error of the definition but the 2^31 list entries (no
    test-sized state has them): the outputs and the struct are untouched, and the context stays usable"""
    import torch
    ctx = gpu_ctx
    name, tol = "bay", (100, 1)
    c, _, b = BY_NAME[name]
    k = cloud(name, tol)
    h, w = c["label"].shape
    nl, n = c["n_labels"], len(k.xyz)
    _, clean, tri = upstream(name, tol)
    d_label, d_top, d_xyz, d_plane = on_device(c["label"], c["top"], k.xyz, k.plane_idx)
    outs = [torch.full((n,), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3)]
    ptrs = [o.data_ptr() for o in outs]
    lp = k.label_plane.ctypes.data

    def stage(out, xyz=d_xyz.data_ptr(), n=n, bin=b, plane=d_plane.data_ptr(), table=lp, clip2=k.clip2, outputs=ptrs, on=ctx):
        return on._L.bs_point_residuals_dev(on._h, xyz, n, bin, plane, table, clip2, *outputs, out)

    def untouched(**kw):
        out = _lib.PointResiduals()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        rc = stage(C.byref(out), **kw)
        msg = kw.get("on", ctx)._L.bs_last_error(kw.get("on", ctx)._h)
        torch.cuda.synchronize()
        assert bytes(out) == b"\x5a" * C.sizeof(out) and all(bool((o == PATTERN).all()) for o in outs), kw
        return rc, msg

    def moved(col, v):
        x = k.xyz.copy()
        x[n // 2, col] = v
        return on_device(x)[0]

    with api.Context(0) as fresh:  # no count
        rc, msg = untouched(on=fresh)
        assert rc == -1 and b"no successful triangle count" in msg
    ctx.outline_triangles_dev(d_label.data_ptr(), 0, w, h, nl, *tol)  # a count without top
    rc, msg = untouched()
    assert rc == -1 and b"no top image" in msg
    ctx.outline_triangles_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, nl, *tol)
    assert stage(None) == -1
    for kw in (dict(xyz=None), dict(n=0), dict(bin=0), dict(clip2=-1), dict(plane=None), dict(table=None)):
        assert untouched(**kw)[0] == -1, kw
    rc, msg = untouched(n=1 << 29)
    assert rc == -2 and b"2^29" in msg
    for col, v, word in ((0, -1, b"negative"), (1, -1, b"negative"), (0, w * b, b"outside"), (1, h * b, b"outside"),
                         (2, 1 << 24, b"2^24"), (2, -(1 << 24), b"2^24")):
        bad = moved(col, v)
        rc, msg = untouched(xyz=bad.data_ptr())
        assert rc == -2 and word in msg, (col, v, msg)
    rc, msg = untouched(bin=(1 << 24) // w + 1)
    assert rc == -2 and b"extent" in msg
    # each output NULL in turn, and all of them; without the plane table; clip2 = 0: the outputs given are written
    want = ref(name, tol)[0]
    for skip in (0, 1, 2, (0, 1, 2)):
        skip = (skip,) if isinstance(skip, int) else skip
        for o in outs:
            o.fill_(PATTERN)
        got = ctx.point_residuals_dev(d_xyz.data_ptr(), n, b, d_plane.data_ptr(), k.label_plane, k.clip2,
                                      *[0 if j in skip else p for j, p in enumerate(ptrs)])
        got.label, got.r2, got.cover = want.label, want.r2, want.cover
        assert pref.same(got, want) is None, pref.same(got, want)
        for j, (o, field) in enumerate(zip(outs, ("label", "r2", "cover"))):
            assert np.array_equal(o.cpu().numpy(), np.full(n, PATTERN) if j in skip else getattr(want, field)), (skip, field)
    for kw in (dict(plane_idx=None, label_plane=None, clip2=k.clip2), dict(plane_idx=k.plane_idx, label_plane=k.label_plane, clip2=0),
               dict(plane_idx=None, label_plane=None, clip2=brute.NO_CLIP2)):
        w2 = pref.point_residuals(clean, tri, nl, w, h, k.xyz, b, **kw)
        g2 = ctx.point_residuals_dev(d_xyz.data_ptr(), n, b, d_plane.data_ptr() if kw["plane_idx"] is not None else 0,
                                     kw["label_plane"], None if kw["clip2"] == brute.NO_CLIP2 else kw["clip2"], *ptrs)
        g2.label, g2.r2, g2.cover = (o.cpu().numpy() for o in outs)
        assert pref.same(g2, w2) is None, (kw["clip2"], pref.same(g2, w2))
    # sz at 2^24: a count over tops of 2^24, a vertex of a triangle is out of range
    high = torch.full_like(d_top, 1 << 24)
    ctx.outline_triangles_dev(d_label.data_ptr(), high.data_ptr(), w, h, nl, *tol)
    for o in outs:
        o.fill_(PATTERN)
    rc, msg = untouched()
    assert rc == -2 and b"vertex" in msg
    with pytest.raises(api.BsError):
        ctx.point_residuals(c["label"], high.cpu().numpy(), k.xyz, n_labels=nl, num=tol[0], den=tol[1], bin=b)
    with pytest.raises(ValueError):
        ctx.point_residuals(c["label"], c["top"], k.xyz, n_labels=nl, bin=b, plane_idx=k.plane_idx)
    check(ctx, name, tol)  # the context stays usable


def test_fidelity_of_a_roof_scene(gpu_ctx):
    """the gabled scene through solid_model -> roof_structure -> point_fidelity at tolerances 0 and 2 px with the planes of
    the segmentation: the figures are the restatement's over the device's own triangles, added up by building"""
    from types import SimpleNamespace
    from test_roofs_cpu import load_roof_scenes
    ctx = gpu_ctx
    xyz = load_roof_scenes().gabled()
    _, _, plane_idx, planes = ctx.segment(xyz, api.default_params(k=15))
    fp, b, roofs, s = ctx.solid_model(xyz, plane_idx, planes, refit=True)
    rf = ctx.roof_structure(b.map, roofs, s)
    pts = np.ascontiguousarray(xyz, dtype=np.int32)  # (the scene is shifted to its origin: the images' own)
    for mm, clip in ((0, None), (2 * s.bin, 100)):
        f, r = ctx.point_fidelity(pts, rf, s, tolerance_mm=mm, plane_idx=plane_idx, clip_mm=clip)
        num, den = api.simplify_tolerance(mm, s.bin)
        gt, gc, _, _ = ctx.outline_triangles(rf.facet, s.top, n_labels=rf.n_facets, num=num, den=den)
        want = pref.point_residuals(gc, gt, rf.n_facets, rf.width, rf.image_height, pts, s.bin, plane_idx, rf.facet_plane,
                                    brute.NO_CLIP2 if clip is None else 2 * clip)
        assert pref.same(r, want, FIGURES) is None, pref.same(r, want, FIGURES)
        wf = api.point_fidelity_of(SimpleNamespace(**vars(want)), rf.facet_building, s.n_buildings)
        for key in ("points", "in_points", "inlier_share", "above_share", "below_share", "bias_mm", "mean_abs_mm", "max_abs_mm",
                    "rmse_mm", "plane_share", "plane_in_share"):
            assert np.array_equal(getattr(f, key), getattr(wf, key)), key
        assert f.n_buildings == s.n_buildings and f.points.sum() + r.n_uncovered == len(pts)
        print("point fidelity: tolerance", mm, "mm, clip", clip, ": points", f.points.tolist(), "inliers", np.round(f.inlier_share, 3).tolist(),
              "bias mm", np.round(f.bias_mm, 1).tolist(), "rmse mm", np.round(f.rmse_mm, 1).tolist(), "plane", np.round(f.plane_share, 3).tolist())
