"""Facet outlines on the device (bs_facet_outlines, bs_facet_outlines_count_dev / _emit_dev; include/bs_api.h) against the
numpy restatement tests/outline_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_outlines_cpu import facet_identity, load_outline_cases  # noqa: E402
from test_roofs_cpu import load_roof_scenes  # noqa: E402

cases = load_outline_cases()
orf, fc = cases.orf, cases.fc

pytestmark = pytest.mark.gpu

NAMED = dict(cases.named_cases())


def check(ctx, c, want=None):
    """the host-memory entry point with top and without against the restatement"""
    want = cases.run_ref(c) if want is None else want
    got = ctx.facet_outlines(c["label"], c["top"], n_labels=c["n_labels"])
    assert orf.same(got, want) is None, orf.same(got, want)
    assert (got.n_labels, got.width, got.image_height) == (c["n_labels"],) + c["label"].shape[::-1]
    flat = ctx.facet_outlines(c["label"], None, n_labels=c["n_labels"])
    assert flat.z is None and not flat.has_z
    flat.z = want.z
    assert orf.same(flat, want) is None, orf.same(flat, want)
    orf.identities(got, c["label"], c["connected"])
    if c["facets"] is not None:
        facet_identity(c, got)
    return got


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case(gpu_ctx, name):
    check(gpu_ctx, NAMED[name])


@pytest.mark.parametrize("w,h", cases.LINE_SIZES)
def test_line_images(gpu_ctx, w, h):
    """1 x 1, 1 x N and N x 1 with N around the wave and beyond one workgroup"""
    check(gpu_ctx, cases.line_case(w, h))


@pytest.mark.parametrize("w,h", fc.SIZES)
def test_image_sizes(gpu_ctx, w, h):
    check(gpu_ctx, cases.from_facet(fc.blob_case(w, h, seed=w * 1000 + h, size=7)))


@pytest.mark.parametrize("seed", range(fc.N_SOLID_FUZZ))
def test_solid_fuzz(gpu_ctx, seed):
    check(gpu_ctx, cases.from_facet(fc.solid_fuzz_case(seed)))


@pytest.mark.parametrize("seed", range(fc.N_FUZZ))
def test_facet_fuzz(gpu_ctx, seed):
    check(gpu_ctx, cases.from_facet(fc.fuzz_case(seed)))


@pytest.mark.parametrize("seed", range(cases.N_RANDOM))
def test_random_labels(gpu_ctx, seed):
    check(gpu_ctx, cases.random_case(seed))


def test_serpentine_one_long_ring(gpu_ctx):
    """one label over 257 x 257 in a single ring of more than 2^16 half-edges: the worst case of the doubling rounds"""
    c = cases.serpentine(257)
    want = cases.run_ref(c)
    assert want.n_rings == 1 and want.ring_length[0] == want.n_half > 1 << 16
    check(gpu_ctx, c, want)


def test_large_image_with_blobs(gpu_ctx):
    """1025 x 1027: more pixels than one sweep of the grid-stride pass (4096 workgroups of 256) and many tiles of the scans
    and the sort"""
    c = cases.from_facet(fc.blob_case(1025, 1027, seed=5, size=40, nb=700))
    assert 1025 * 1027 > 4096 * 256
    want = cases.run_ref(c)
    assert want.n_half > 16 * 4096 and want.n_rings > 1000
    check(gpu_ctx, c, want)


def test_no_labelled_pixel(gpu_ctx):
    c = cases.from_facet(fc.solid_fuzz_case(15))
    assert (c["label"] < 0).all()
    got = check(gpu_ctx, c)
    assert (got.n_half, got.n_rings, got.n_vertices) == (0, 0, 0) and got.ring_offset.tolist() == [0]
    assert (got.label_ring_offset == 0).all() and got.xy.shape == (0, 2)


# ---- device pointers --------------------------------------------------------------------------------------------------
PATTERN = -0x5A5A5A5B  # no lattice coordinate and no top of the cases


def dev_run(ctx, c, with_top):
    import torch
    h, w = c["label"].shape
    d_label = torch.from_numpy(c["label"]).cuda()
    d_top = torch.from_numpy(c["top"]).cuda() if with_top else None
    torch.cuda.synchronize()  # (the context has a stream of its own)
    o = ctx.facet_outlines_dev(d_label.data_ptr(), d_top.data_ptr() if with_top else 0, w, h, c["n_labels"])
    assert o.xy is None and o.z is None and o.has_z == with_top
    outs = []
    for _ in range(2):  # the emit may be called more than once
        d_xy = torch.full((o.n_vertices, 2), PATTERN, dtype=torch.int32, device="cuda")
        d_z = torch.full((o.n_vertices,), PATTERN, dtype=torch.int32, device="cuda") if with_top else None
        torch.cuda.synchronize()
        ctx.facet_outlines_emit_dev(d_xy.data_ptr(), d_z.data_ptr() if with_top else 0)
        outs.append((d_xy.cpu().numpy(), d_z.cpu().numpy() if with_top else None))
    (xy, z), (xy2, z2) = outs
    assert (xy != PATTERN).all() and np.array_equal(xy, xy2)  # every element is written, and twice the same
    if with_top:
        assert (z != PATTERN).all() and np.array_equal(z, z2)
    o.xy, o.z = xy, z
    return o


def test_device_pointers(gpu_ctx):
    for c in (cases.from_facet(fc.fuzz_case(1)), cases.from_facet(fc.solid_fuzz_case(3))):  # one context: the scratch is reused
        want = cases.run_ref(c)
        for with_top in (True, False):
            got = dev_run(gpu_ctx, c, with_top)
            if not with_top:
                got.z = want.z
            assert orf.same(got, want) is None, orf.same(got, want)


# ---- errors -----------------------------------------------------------------------------------------------------------
def raw(ctx, c, dev, **kw):
    """bs_facet_outlines_count_dev on the device pointers dev = (d_label, d_top), single arguments replaced by kw: returns
    (status, the bs_outlines, which was filled with a pattern before the call)"""
    h, w = c["label"].shape
    a = dict(d_label=dev[0], d_top=dev[1], width=w, height=h, n_labels=c["n_labels"], out=True)
    a.update(kw)
    out = _lib.Outlines()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    rc = ctx._L.bs_facet_outlines_count_dev(ctx._h, a["d_label"] or None, a["d_top"] or None, a["width"], a["height"],
                                            a["n_labels"], C.byref(out) if a["out"] else None)
    return rc, out


def untouched_struct(out):
    return bytes(out) == b"\x5a" * C.sizeof(out)


def test_error_paths(gpu_ctx):
    import torch
    ctx = gpu_ctx
    c = cases.from_facet(fc.fuzz_case(5))
    want = cases.run_ref(c)
    d_label, d_top = torch.from_numpy(c["label"]).cuda(), torch.from_numpy(c["top"]).cuda()
    d_xy = torch.full((want.n_vertices, 2), PATTERN, dtype=torch.int32, device="cuda")
    d_z = torch.full((want.n_vertices,), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    dev = (d_label.data_ptr(), d_top.data_ptr())
    emit = lambda: ctx._L.bs_facet_outlines_emit_dev(ctx._h, d_xy.data_ptr(), d_z.data_ptr())  # noqa: E731

    def untouched():
        torch.cuda.synchronize()
        return bool((d_xy == PATTERN).all()) and bool((d_z == PATTERN).all())

    def good():
        """a following good call equals the reference"""
        rc, out = raw(ctx, c, dev)
        assert rc == 0 and (out.n_half, out.n_rings, out.n_vertices) == (want.n_half, want.n_rings, want.n_vertices)
        ctx._L.bs_outlines_free(C.byref(out))
        xy, z = torch.empty_like(d_xy), torch.empty_like(d_z)
        torch.cuda.synchronize()
        ctx.facet_outlines_emit_dev(xy.data_ptr(), z.data_ptr())
        assert np.array_equal(xy.cpu().numpy(), want.xy) and np.array_equal(z.cpu().numpy(), want.z)

    # an emit before any count, on a context of its own
    with api.Context(0) as fresh:
        assert fresh._L.bs_facet_outlines_emit_dev(fresh._h, d_xy.data_ptr(), d_z.data_ptr()) == -1
    assert untouched()
    # BS_ERR_INVALID from the arguments: 2^15 x 2^14 is refused before anything is read (the buffers are far smaller)
    for kw in (dict(width=1 << 15, height=1 << 14), dict(d_label=0), dict(out=False), dict(width=0), dict(height=0),
               dict(width=-3), dict(height=-1), dict(n_labels=-1), dict(d_top=dev[1] + 4)):
        good()
        rc, out = raw(ctx, c, dev, **kw)
        assert rc == -1, kw
        assert untouched_struct(out), kw
        assert emit() == -1 and untouched(), kw  # an emit after a failed count
    assert b"facet outlines" in ctx._L.bs_last_error(ctx._h)
    # BS_ERR_RANGE: a label >= n_labels
    good()
    lab = c["label"].copy()
    lab[tuple(np.argwhere(lab >= 0)[0])] = c["n_labels"]
    d_bad = torch.from_numpy(lab).cuda()
    torch.cuda.synchronize()
    rc, out = raw(ctx, c, (d_bad.data_ptr(), dev[1]))
    assert rc == -2 and untouched_struct(out)
    assert emit() == -1 and untouched()
    with pytest.raises(api.BsError) as e:  # the host-memory twin reports the same
        ctx.facet_outlines(lab, c["top"], n_labels=c["n_labels"])
    assert e.value.status == -2
    # d_z against the count: given without top, missing with top
    good()
    assert ctx._L.bs_facet_outlines_emit_dev(ctx._h, d_xy.data_ptr(), None) == -1 and untouched()
    rc, out = raw(ctx, c, (dev[0], 0))
    assert rc == 0
    ctx._L.bs_outlines_free(C.byref(out))
    assert emit() == -1 and untouched()
    # the context is as usable as before
    good()
    check(ctx, cases.from_facet(fc.fuzz_case(2)))


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_gabled_scene_end_to_end(gpu_ctx, tmp_path):
    sc = load_roof_scenes()
    xyz = sc.gabled()
    _, _, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=15))
    fp, b, r, s = gpu_ctx.solid_model(xyz, plane_idx, planes, refit=True)
    rf = gpu_ctx.roof_structure(b.map, r, s)
    o = gpu_ctx.roof_outlines(rf, s)
    c = dict(label=rf.facet, top=s.top, n_labels=rf.n_facets, connected=True, facets=rf)
    want = cases.run_ref(c)
    assert orf.same(o, want) is None, orf.same(o, want)
    orf.identities(o, rf.facet, True)
    print("gable: facets", rf.n_facets, "half-edges", o.n_half, "rings", o.n_rings, "vertices", o.n_vertices)
    # the real stage's own figures: boundary length and start pixel of every facet
    per = np.zeros(rf.n_facets, np.int64)
    np.add.at(per, o.ring_label, o.ring_length)
    assert np.array_equal(per, rf.facet_inner_edges + rf.facet_outer_edges)
    start = rf.facet_start_xy[:, 1].astype(np.int64) * rf.width + rf.facet_start_xy[:, 0]
    assert np.array_equal(o.ring_start[o.label_ring_offset[:-1]], 4 * start)
    # Z at every vertex = top read from ANY pixel of the facet at that corner
    lab = np.repeat(o.ring_label, o.ring_vertices)
    h, w = rf.facet.shape
    seen = np.zeros(o.n_vertices, np.int64)
    for (ox, oy), t in (((-1, -1), 3), ((0, -1), 2), ((-1, 0), 1), ((0, 0), 0)):  # the pixel at this offset has the corner as t
        px, py = o.xy[:, 0] + ox, o.xy[:, 1] + oy
        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        ok[ok] = rf.facet[py[ok], px[ok]] == lab[ok]
        assert np.array_equal(s.top[py[ok], px[ok], t], o.z[ok])
        seen += ok
    assert (seen >= 1).all()
    with pytest.raises(ValueError):
        gpu_ctx.roof_outlines(api.RoofFacets(**{**vars(rf), "facet": None}), s)
    api.write_outlines_obj(o, tmp_path / "outlines.obj", 100, origin=(0, 0, 0))
    assert open(tmp_path / "outlines.obj", "rb").read() == cases.brute.obj_text(want, 100, (0, 0, 0))
