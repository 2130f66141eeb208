"""Outline triangles on the device (bs_outline_triangles, bs_outline_triangles_count_dev / _emit_dev; include/bs_api.h)
against the numpy restatement tests/triangulate_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_roofs_cpu import load_roof_scenes  # noqa: E402
from test_triangulate_cpu import RUNS, check_identities, load_triangulate_cases, ref  # noqa: E402

cases = load_triangulate_cases()
tref, brute, uref = cases.tref, cases.brute, cases.uref

pytestmark = pytest.mark.gpu

PATHS = dict.fromkeys(tref.PATHS, 0)  # labels by kernel path over everything this module has run


def check(ctx, name, tol, with_top=True):
    """the host-memory entry point against the restatement: every array and total"""
    c = RUNS[name][0]
    plain, clean, want = ref(name, tol)
    got, gc, gs, gp = ctx.outline_triangles(c["label"], c["top"] if with_top else None, n_labels=c["n_labels"], num=tol[0], den=tol[1])
    assert tref.same(got, want) is None, (name, tol, tref.same(got, want))
    assert (got.wave_cap, got.lds_cap) == (tref.WAVE_CAP, tref.LDS_CAP) == (_lib.TRI_WAVE_CAP, _lib.TRI_LDS_CAP)
    assert (got.n_rings, got.n_svertices) == (clean.n_rings, clean.n_svertices)
    assert np.array_equal(gc.sxy, clean.sxy) and np.array_equal(gc.s_ring_offset, clean.s_ring_offset)
    assert (gc.sz is not None) == with_top and (not with_top or np.array_equal(gc.sz, clean.sz))
    assert gs.sxy is None and gp.xy is None and np.array_equal(gp.ring_area2, plain.ring_area2)
    for k in PATHS:
        PATHS[k] += getattr(got, k)
    return got, gc, gp


@pytest.mark.parametrize("name", sorted(RUNS))
def test_case(gpu_ctx, name):
    """every case at every tolerance of its own"""
    for i, tol in enumerate(RUNS[name][1]):
        check(gpu_ctx, name, tol, with_top=i % 2 == 0)


def test_all_three_paths_ran_and_the_comb_walks(gpu_ctx):
    """a wave per label, a workgroup with LDS, a workgroup with the global workspace; the comb's scan really walks"""
    check(gpu_ctx, "nested", (0, 1))
    check(gpu_ctx, "sieve_24", (0, 1))
    got, gc, gp = check(gpu_ctx, "long_comb", (0, 1))
    assert got.max_label_occurrences > got.lds_cap and (got.n_labels_wave, got.n_labels_lds, got.n_labels_global) == (0, 0, 1)
    assert all(PATHS[k] > 0 for k in PATHS), PATHS
    comb, gc, gp = check(gpu_ctx, "comb_300", (0, 1))
    assert comb.n_tests > 10 * comb.n_triangles and comb.n_triangles == 1202
    check_identities(gp, gc, comb, False)
    print("comb_300: tests per triangle", comb.n_tests / comb.n_triangles, comb.info)


def test_no_bridge_label_on_the_device(gpu_ctx):
    (name, tol, l), = cases.NO_BRIDGE_RUNS
    got, gc, gp = check(gpu_ctx, name, tol)
    assert got.label_status[l] == brute.NO_BRIDGE and got.n_failed_labels == 1
    assert (got.tri[got.tri_offset[l]:got.tri_offset[l + 1]] == -1).all() and got.tri_offset[l + 1] > got.tri_offset[l]
    check_identities(gp, gc, got, True)


PATTERN = -0x5A5A5A5B


def test_device_pointers_and_errors(gpu_ctx):
    import torch
    ctx = gpu_ctx
    name, tol = "sieve_30", (0, 1)
    c = RUNS[name][0]
    plain, clean, want = ref(name, tol)
    h, w = c["label"].shape
    d_label, d_top = torch.from_numpy(c["label"]).cuda(), torch.from_numpy(c["top"]).cuda()
    d_tri = torch.full((want.n_triangles, 3), PATTERN, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with api.Context(0) as fresh:  # an emit without a count
        assert fresh._L.bs_outline_triangles_emit_dev(fresh._h, d_tri.data_ptr()) == -1
        assert b"without a successful count" in fresh._L.bs_last_error(fresh._h)

    def count(out, tolerance=tol, cell_log2=0):
        return ctx._L.bs_outline_triangles_count_dev(ctx._h, d_label.data_ptr(), d_top.data_ptr(), w, h, c["n_labels"], tolerance[0],
                                                     tolerance[1], cell_log2, out, None, None, None)

    assert count(None) == -1  # a null result
    for bad in ((1, 0), (-1, 1), (1 << 31, 1)):  # a bad tolerance: the output stays untouched
        out = _lib.OutlineTriangles()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        assert count(C.byref(out), bad) == -1 and bytes(out) == b"\x5a" * C.sizeof(out)
    out = _lib.OutlineTriangles()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    assert count(C.byref(out), cell_log2=31) == -1 and bytes(out) == b"\x5a" * C.sizeof(out)
    assert ctx._L.bs_outline_triangles_emit_dev(ctx._h, d_tri.data_ptr()) == -1  # a failed count leaves nothing to emit
    with pytest.raises(api.BsError):
        ctx.outline_triangles(c["label"], c["top"], n_labels=c["n_labels"], num=1, den=0)
    got, gc, gs, gp = ctx.outline_triangles_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, c["n_labels"], *tol)
    assert got.tri is None and gc.sxy is None and got.n_triangles == want.n_triangles
    assert ctx._L.bs_outline_triangles_emit_dev(ctx._h, None) == -1  # a missing buffer
    torch.cuda.synchronize()
    assert bool((d_tri == PATTERN).all())
    first = None
    for _ in range(2):  # the emit twice: the same bytes
        d_tri.fill_(PATTERN)
        ctx.outline_triangles_emit_dev(d_tri.data_ptr())
        b = d_tri.cpu().numpy().tobytes()
        assert first is None or b == first
        first = b
    got.tri = d_tri.cpu().numpy()
    assert tref.same(got, want) is None, tref.same(got, want)
    # the clean vertices of the same count are still there for their own emit
    d_xy = torch.zeros((clean.n_svertices, 2), dtype=torch.int32, device="cuda")
    d_z = torch.zeros((clean.n_svertices,), dtype=torch.int32, device="cuda")
    d_right = torch.zeros((clean.n_svertices,), dtype=torch.int32, device="cuda")
    d_flag = torch.zeros((clean.n_svertices,), dtype=torch.uint8, device="cuda")
    ctx.clean_outlines_emit_dev(d_xy.data_ptr(), d_z.data_ptr(), d_right.data_ptr(), d_flag.data_ptr())
    assert np.array_equal(d_xy.cpu().numpy(), clean.sxy)


def test_no_labelled_pixel(gpu_ctx):
    lab = np.full((3, 4), -1, np.int32)
    got, gc, gs, gp = gpu_ctx.outline_triangles(lab, None, n_labels=2)
    assert got.n_triangles == 0 and got.tri.shape == (0, 3) and (got.label_status == brute.EMPTY).all()
    assert np.array_equal(got.tri_offset, [0, 0, 0]) and got.n_labels_wave == 0


def test_writer_against_the_reference_text(gpu_ctx, tmp_path):
    for name, tol in (("nested", (0, 1)),) + tuple((n, t) for n, t, _ in cases.NO_BRIDGE_RUNS):
        c = RUNS[name][0]
        plain, clean, want = ref(name, tol)
        got, gc, _, _ = gpu_ctx.outline_triangles(c["label"], c["top"], n_labels=c["n_labels"], num=tol[0], den=tol[1])
        api.write_outline_triangles_obj(got, gc, tmp_path / "t.obj", 25, origin=(1000, -2000, 30))
        text = open(tmp_path / "t.obj", "rb").read()
        assert text == brute.obj_text(brute.triangulate(plain, clean), clean, 25, (1000, -2000, 30))
    assert text.startswith(b"# outline triangles: ") and b" 1 failed labels, " in text.split(b"\n")[0]
    with pytest.raises(api.BsError):
        api.write_outline_triangles_obj(got, gc, tmp_path / "t.obj", 0)
    with pytest.raises(api.BsError):
        api.write_outline_triangles_obj(got, gc, tmp_path / "no_such_dir" / "t.obj", 25)


def test_gabled_scene_roof_mesh(gpu_ctx):
    sc_ = load_roof_scenes()
    xyz = sc_.gabled()
    _, _, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=15))
    fp, b, r, s = gpu_ctx.solid_model(xyz, plane_idx, planes, refit=True)
    rf = gpu_ctx.roof_structure(b.map, r, s)
    for mm in (0, 400):
        t, o, plain = gpu_ctx.roof_mesh(rf, s, tolerance_mm=mm)
        num, den = api.simplify_tolerance(mm, s.bin)
        wp, _, wc = uref.clean(rf.facet, s.top, rf.n_facets, num, den)
        want = tref.triangulate(wp, wc)
        assert tref.same(t, want) is None, tref.same(t, want)
        assert mm > 0 or (t.n_failed_labels == 0 and (t.label_status == brute.OK).all())  # (every node kept: nothing sweeps)
        check_identities(plain, o, t, False)
        o2, _ = gpu_ctx.roof_polygons(rf, s, tolerance_mm=mm, clean=True)  # the mesh stands on exactly these vertices
        assert np.array_equal(o2.sxy, o.sxy) and np.array_equal(o2.s_ring_offset, o.s_ring_offset)
        print("gable: tolerance", mm, "mm: triangles", t.n_triangles, "bridges", t.n_bridges, "tests", t.n_tests, "largest label",
              t.max_label_occurrences)
