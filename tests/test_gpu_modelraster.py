"""Model raster on the device (bs_model_raster, bs_model_raster_dev; include/bs_api.h) against the numpy restatement
tests/modelraster_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_roofs_cpu import load_roof_scenes  # noqa: E402
from test_modelraster_cpu import BY_NAME, load_modelraster_cases, ref, upstream  # noqa: E402

cases = load_modelraster_cases()
mref, brute, tref = cases.mref, cases.brute, cases.tref

pytestmark = pytest.mark.gpu
PATTERN = -0x5A5A5A5B


def check(ctx, name, tol):
    """the host-memory entry point against the restatement over the restated stages before: all three images and every
    figure"""
    c = BY_NAME[name][0]
    want = ref(name, tol)[0]
    _, clean, tri = upstream(name, tol)
    got, gt, gc, gs, gp = ctx.model_raster(c["label"], c["top"], n_labels=c["n_labels"], num=tol[0], den=tol[1])
    assert mref.same(got, want) is None, (name, tol, mref.same(got, want))
    assert (got.fig_cap, got.chunk) == (mref.FIG_CAP, mref.CHUNK)
    assert tref.same(gt, tri) is None and np.array_equal(gc.sxy, clean.sxy) and np.array_equal(gc.sz, clean.sz)
    return got


def against_own_upstream(ctx, label, top, tol=(0, 1), n_labels=None):
    """the device against the restatement of this stage over the device's own clean outlines and triangles (the stages before
    have their own tests): for images too large for the restatements of the whole chain"""
    got, gt, gc, _, _ = ctx.model_raster(label, top, n_labels=n_labels, num=tol[0], den=tol[1])
    want = mref.model_raster(gc, gt, label, top, got.n_labels)
    assert mref.same(got, want) is None, mref.same(got, want)
    return got, gt, gc


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_case(gpu_ctx, name):
    """every named run at every tolerance of its own; the bay, the staircase, wide, band, the strips round the cap of the
    figure tables, the image without a labelled pixel and the NO_BRIDGE run are names of this list"""
    for tol in BY_NAME[name][1]:
        check(gpu_ctx, name, tol)


def test_shapes_on_the_device(gpu_ctx):
    """what the shapes are for, read from the device's result"""
    r = check(gpu_ctx, "bay", (100, 1))
    assert (r.n_multi, r.n_spill, r.n_moved) == (1, 31, 1) and r.model[4, 7] == 0 and r.cover[4, 7] == 2
    for n in cases.STRIPS:
        s = check(gpu_ctx, f"strip_{n}", (0, 1))
        assert (s.kept == 1).all() and len(s.kept) == n
    (name, tol, l), = cases.tc.NO_BRIDGE_RUNS
    f = check(gpu_ctx, name, tol)
    assert f.model_pixels[l] == 0 and f.pixels[l] > 0 and not (f.model == l).any()
    e = check(gpu_ctx, "no_label_pixel", (0, 1))
    assert e.total_pixels == 0 and (e.model == -1).all() and (e.cover == 0).all() and (e.mz2 == brute.INT32_MIN).all()


def test_wide_and_band(gpu_ctx):
    """spans longer than a workgroup's chunk of pixel items; slivers with rows that hold no pixel centre"""
    w = check(gpu_ctx, "wide", (0, 1))
    assert w.max_span > w.chunk and w.n_items > 64 * w.chunk and w.total_kept == 3000 * 40
    b = check(gpu_ctx, "band", (2, 1))
    assert b.n_empty_spans > 0 and b.n_rows > 1000 and b.max_span <= 4
    print("wide:", w.n_rows, w.n_items, w.max_span, "band:", b.n_rows, b.n_items, b.n_empty_spans, b.max_span)


def test_reads_the_state_and_leaves_it(gpu_ctx):
    """poly_solids_dev, then model_raster_dev, then poly_solids_emit_dev: the mesh is byte-identical to an emit without the
    raster in between, and the raster equals the host-memory entry point"""
    import torch
    ctx = gpu_ctx
    name, tol = "nested", (2, 1)
    c = BY_NAME[name][0]
    h, w = c["label"].shape
    nl = c["n_labels"]
    lb = (np.arange(nl) % 3).astype(np.int32)
    d_label, d_top, d_lb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["label"], c["top"], lb))

    def mesh(raster):
        s = ctx.poly_solids_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, nl, d_lb.data_ptr(), 3, *tol, bin=25, base_z=-1000)[0]
        bufs = [torch.full(shape, PATTERN if dt != torch.uint8 else 0xA5, dtype=dt, device="cuda")
                for shape, dt in (((s.n_vertices, 4), torch.int32), ((s.n_faces + 1,), torch.int32), ((s.n_indices,), torch.int32),
                                  ((s.n_faces,), torch.int32), ((s.n_faces,), torch.uint8))]
        imgs = [torch.full((h, w), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3)]
        r = ctx.model_raster_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, *[i.data_ptr() for i in imgs]) if raster else None
        ctx.poly_solids_emit_dev(*[b.data_ptr() for b in bufs])
        d_tri = torch.zeros((upstream(name, tol)[2].n_triangles, 3), dtype=torch.int32, device="cuda")
        ctx.outline_triangles_emit_dev(d_tri.data_ptr())
        return b"".join(x.cpu().numpy().tobytes() for x in bufs + [d_tri]), r, [i.cpu().numpy() for i in imgs]

    plain, _, _ = mesh(False)
    with_raster, r, imgs = mesh(True)
    assert plain == with_raster
    r.model, r.cover, r.mz2 = imgs
    assert mref.same(r, ref(name, tol)[0]) is None, mref.same(r, ref(name, tol)[0])


def test_null_images_and_errors(gpu_ctx):
    import torch
    ctx = gpu_ctx
    name, tol = "bay", (100, 1)
    c = BY_NAME[name][0]
    want = ref(name, tol)[0]
    h, w = c["label"].shape
    nl = c["n_labels"]
    d_label, d_top = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["label"], c["top"]))
    imgs = [torch.full((h, w), PATTERN, dtype=torch.int32, device="cuda") for _ in range(3)]
    ptrs = [i.data_ptr() for i in imgs]

    def raster(out, label=d_label.data_ptr(), top=d_top.data_ptr(), width=w, height=h, images=ptrs, on=ctx):
        return on._L.bs_model_raster_dev(on._h, label, top, width, height, *images, out)

    def untouched(**kw):
        out = _lib.ModelRaster()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        rc = raster(C.byref(out), **kw)
        msg = kw.get("on", ctx)._L.bs_last_error(kw.get("on", ctx)._h)
        torch.cuda.synchronize()
        assert bytes(out) == b"\x5a" * C.sizeof(out) and all(bool((i == PATTERN).all()) for i in imgs)
        return rc, msg

    with api.Context(0) as fresh:  # no count
        rc, msg = untouched(on=fresh)
        assert rc == -1 and b"no successful triangle count" in msg
    ctx.outline_triangles_dev(d_label.data_ptr(), 0, w, h, nl, *tol)  # a count without top
    rc, msg = untouched()
    assert rc == -1 and b"no top image" in msg
    ctx.outline_triangles_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, nl, *tol)
    assert raster(None) == -1 and untouched(label=None)[0] == -1 and untouched(top=None)[0] == -1
    rc, msg = untouched(width=w - 1)  # a size mismatch
    assert rc == -1 and b"size" in msg
    assert untouched(width=h, height=w + 1)[0] == -1
    high = torch.full_like(d_top, 1 << 24)  # |t00 + t11| = 2^25 on the pixels where e2 is formed
    rc, msg = untouched(top=high.data_ptr())
    assert rc == -2 and b"2^25" in msg
    # each image NULL in turn, and all of them: the figures are the same, the images given are written
    for skip in (0, 1, 2, (0, 1, 2)):
        skip = (skip,) if isinstance(skip, int) else skip
        for i in imgs:
            i.fill_(PATTERN)
        got = ctx.model_raster_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, *[0 if k in skip else p for k, p in enumerate(ptrs)])
        got.model, got.cover, got.mz2 = want.model, want.cover, want.mz2
        assert mref.same(got, want) is None, mref.same(got, want)
        for k, (img, field) in enumerate(zip(imgs, ("model", "cover", "mz2"))):
            assert np.array_equal(img.cpu().numpy(), np.full((h, w), PATTERN) if k in skip else getattr(want, field)), (skip, field)
    # sz at 2^24: a count over tops of 2^24, a vertex of a triangle is out of range
    ctx.outline_triangles_dev(d_label.data_ptr(), high.data_ptr(), w, h, nl, *tol)
    for i in imgs:
        i.fill_(PATTERN)
    rc, msg = untouched(top=d_top.data_ptr())
    assert rc == -2 and b"2^24" in msg
    with pytest.raises(api.BsError):
        ctx.model_raster(c["label"], high.cpu().numpy(), n_labels=nl, num=tol[0], den=tol[1])
    assert _lib.STATUS[-2] == "BS_ERR_RANGE" and _lib.STATUS[-1] == "BS_ERR_INVALID"
    check(ctx, name, tol)  # the context stays usable


def test_noise_crosses_every_sweep_and_tile(gpu_ctx):
    """random labels per pixel, 600 x 600 (the polygon solids' noise recipe): the grid-stride passes over the triangles and
    the row items take 1024 workgroups of 256, so one sweep is 262 144 items -- the triangles, the row items and the pixel
    items all exceed it, and with it one tile of the scans; labels far beyond the cap of the figure tables.  (The pass over
    the pixels takes 2048 workgroups: test_figures_pass_takes_a_second_sweep.)"""
    rng = np.random.default_rng(77)
    nl = 50000
    lab = rng.integers(-1, nl, (600, 600)).astype(np.int32)
    top = rng.integers(-500, 500, (600, 600, 4)).astype(np.int32)
    r, t, c = against_own_upstream(gpu_ctx, lab, top, n_labels=nl)
    print("noise: triangles", t.n_triangles, "rows", r.n_rows, "items", r.n_items, "empty spans", r.n_empty_spans, r.info)
    assert r.n_rows > 262144 and r.n_items > 262144 and t.n_triangles > 262144
    assert r.n_uncovered == r.n_spill == r.n_moved == r.n_multi == 0 and r.model_pixels[mref.FIG_CAP:].sum() > 0


def test_figures_pass_takes_a_second_sweep(gpu_ctx):
    """750 x 800 of blobs: more pixels than one sweep of the pass over the pixels (BS_MRASTER_FIG_GRID workgroups of 256), so
    some of its threads take a second pixel with their register totals and LDS tables kept; blobs of no label
    leave whole waves with nothing to add in every sweep, and labels lie on both sides of the cap of the figure tables"""
    rng = np.random.default_rng(79)
    nl = 3 * mref.FIG_CAP
    coarse = rng.integers(-1, nl, (30, 32)).astype(np.int32)
    coarse[rng.random(coarse.shape) < 0.25] = -1
    lab = np.kron(coarse, np.ones((25, 25), np.int32)).astype(np.int32)
    lab[rng.random(lab.shape) < 0.01] = -1
    top = rng.integers(-500, 500, lab.shape + (4,)).astype(np.int32)
    sweep = 256 * _lib.MRASTER_FIG_GRID
    assert sweep < lab.size < 2 * sweep  # (one sweep and a part of a second)
    for tol in ((0, 1), (4, 1)):
        r, _, _ = against_own_upstream(gpu_ctx, lab, top, tol, n_labels=nl)
        assert r.width * r.height == lab.size > sweep and r.total_pixels > sweep // 2
        assert r.model_pixels[:mref.FIG_CAP].sum() > 0 and r.model_pixels[mref.FIG_CAP:].sum() > 0


def test_blobs_keep_waves_inside_one_label(gpu_ctx):
    """large blobs at a tolerance: whole waves of pixels inside one label of the image and one of the model (the register
    path of the figures), beside waves that straddle a moved boundary"""
    rng = np.random.default_rng(78)
    coarse = rng.integers(-1, 40, (12, 16)).astype(np.int32)
    lab = np.kron(coarse, np.ones((25, 25), np.int32)).astype(np.int32)
    lab[rng.random(lab.shape) < 0.02] = -1
    top = rng.integers(-500, 500, lab.shape + (4,)).astype(np.int32)
    for tol in ((0, 1), (4, 1)):
        r, _, _ = against_own_upstream(gpu_ctx, lab, top, tol, n_labels=40)
        assert r.total_kept > 64 * 40


def test_fidelity_of_a_roof_scene(gpu_ctx):
    """the gabled scene through solid_model -> roof_structure -> model_fidelity at tolerances 0 and 2 px: at 0 nothing is
    lost, gained or covered twice in any building; at both the figures are the restatement's, added up by building"""
    ctx = gpu_ctx
    xyz = load_roof_scenes().gabled()
    _, _, plane_idx, planes = ctx.segment(xyz, api.default_params(k=15))
    fp, b, roofs, s = ctx.solid_model(xyz, plane_idx, planes, refit=True)
    rf = ctx.roof_structure(b.map, roofs, s)
    for mm in (0, 2 * s.bin):
        f, r = ctx.model_fidelity(rf, s, tolerance_mm=mm)
        num, den = api.simplify_tolerance(mm, s.bin)
        gt, gc, _, _ = ctx.outline_triangles(rf.facet, s.top, n_labels=rf.n_facets, num=num, den=den)
        want = mref.model_raster(gc, gt, rf.facet, s.top, rf.n_facets)
        assert mref.same(r, want) is None, mref.same(r, want)
        wf = api.model_fidelity_of(SimpleNamespace(**vars(want)), rf.facet_building, s.n_buildings)
        for k in ("pixels", "lost", "gained", "twice", "err_pixels", "mean_abs_mm", "max_abs_mm", "rmse_mm"):
            assert np.array_equal(getattr(f, k), getattr(wf, k)), k
        assert f.n_buildings == s.n_buildings and f.pixels.sum() == (rf.facet >= 0).sum()
        if mm == 0:
            assert not f.lost.any() and not f.gained.any() and not f.twice.any()
        print("fidelity: tolerance", mm, "mm: lost", f.lost.tolist(), "gained", f.gained.tolist(), "twice", f.twice.tolist(),
              "rmse mm", np.round(f.rmse_mm, 2).tolist(), "max mm", f.max_abs_mm.tolist())
