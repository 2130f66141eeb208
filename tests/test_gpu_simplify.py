"""Simplified outlines on the device (bs_simple_outlines, bs_simple_outlines_count_dev / _emit_dev; include/bs_api.h)
against the numpy restatement tests/simplify_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_roofs_cpu import load_roof_scenes  # noqa: E402
from test_simplify_cpu import load_simplify_cases, twin_identity  # noqa: E402

cases = load_simplify_cases()
sref, oc, fc = cases.sref, cases.oc, cases.fc
orf = oc.orf

pytestmark = pytest.mark.gpu

NAMED = dict(cases.named_cases())
PLAIN_FIELDS = [f for f in orf.brute.FIELDS if f not in ("xy", "z")]


def same_plain(got, want):
    for f in PLAIN_FIELDS:
        if not np.array_equal(np.asarray(getattr(got, f), np.int64), np.asarray(getattr(want, f), np.int64)):
            return f
    return None


def check(ctx, c, tol, want=None):
    """the host-memory entry point with top and without against the restatement, every array, figure and total"""
    plain, want = cases.run_ref(c, tol) if want is None else want
    for with_top in (True, False):
        got, gp = ctx.simplified_outlines(c["label"], c["top"] if with_top else None, n_labels=c["n_labels"], num=tol[0],
                                          den=tol[1])
        assert got.has_z == with_top and (got.sz is not None) == with_top
        if not with_top:
            got.sz = want.sz
        assert sref.same(got, want) is None, (tol, with_top, sref.same(got, want))
        assert (got.n_labels, got.width, got.image_height) == (c["n_labels"],) + c["label"].shape[::-1]
        assert (got.tol_num, got.tol_den) == tol
        assert same_plain(gp, plain) is None, (tol, same_plain(gp, plain))
        assert np.array_equal(got.ring_label, plain.ring_label) and np.array_equal(got.ring_area2, plain.ring_area2)
        assert np.array_equal(got.label_ring_offset, plain.label_ring_offset)
    return got, gp


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case(gpu_ctx, name):
    """the named shapes, the line images, the 16 facet fuzz cases and the 60 random images at every tolerance"""
    for tol in cases.TOLERANCES:
        check(gpu_ctx, NAMED[name], tol)


def test_plain_equals_facet_outlines(gpu_ctx):
    """the plain struct is what bs_facet_outlines returns on the same images"""
    for name in ("fuzz_3", "random_7", "saddle_joined", "nothing"):
        c = NAMED[name]
        _, gp = gpu_ctx.simplified_outlines(c["label"], c["top"], n_labels=c["n_labels"], num=1, den=1)
        o = gpu_ctx.facet_outlines(c["label"], c["top"], n_labels=c["n_labels"])
        assert same_plain(gp, o) is None and gp.xy is None


@pytest.mark.parametrize("name,c,tols", list(cases.big_cases()), ids=[b[0] for b in cases.big_cases()])
def test_products_beyond_64_bits(gpu_ctx, name, c, tols):
    """the one-pixel L and U of 400 x 400 with den = 2^31 - 1: in the U c^2 * den passes 2^64 where the tolerance decides
    (the L's large corner is its arc's forced first split)"""
    kept = []
    for tol in tols:
        t = {}
        want = cases.run_ref(c, tol, t)
        if tol[1] == cases.BIG_DEN and name == "thin_u_400":
            assert t["max_product"] >= 1 << 64
        kept.append(check(gpu_ctx, c, tol, want)[0].n_svertices)
    assert len(set(kept)) > 1


def test_large_image_with_blobs(gpu_ctx):
    """1025 x 1027 at tolerance (1, 1): more pixels than one sweep of the grid-stride passes, more than 1000 rings"""
    c = oc.from_facet(fc.blob_case(1025, 1027, seed=5, size=40, nb=700))
    assert 1025 * 1027 > 4096 * 256
    want = cases.run_ref(c, (1, 1))
    assert want[0].n_half > 16 * 4096 and want[0].n_rings > 1000
    got, _ = gpu_ctx.simplified_outlines(c["label"], c["top"], n_labels=c["n_labels"], num=1, den=1)
    assert sref.same(got, want[1]) is None, sref.same(got, want[1])
    print("blobs: nodes", got.n_nodes, "arcs", got.n_arcs, "rounds", got.rounds, "vertices", got.n_svertices)


def test_noise_crosses_the_node_sweeps(gpu_ctx):
    """512 x 512 of noise: more half-edges and more nodes than one sweep of the stage's own grid-stride passes (1024
    workgroups of 256), and more than 2^16 rings"""
    rng = np.random.default_rng(11)
    lab = rng.integers(-1, 3, (512, 512)).astype(np.int32)
    top = rng.integers(-500, 500, (512, 512, 4)).astype(np.int32)
    plain, want = sref.simplify(lab, top, 3, 1, 1)
    assert want.n_nodes > 2 * 1024 * 256 and plain.n_rings > 1 << 16
    got, gp = gpu_ctx.simplified_outlines(lab, top, n_labels=3, num=1, den=1)
    assert sref.same(got, want) is None, sref.same(got, want)
    assert same_plain(gp, plain) is None


# ---- device pointers --------------------------------------------------------------------------------------------------
PATTERN = -0x5A5A5A5B  # no lattice coordinate, label or top of the cases


def dev_run(ctx, c, tol, with_top):
    import torch
    h, w = c["label"].shape
    d_label = torch.from_numpy(c["label"]).cuda()
    d_top = torch.from_numpy(c["top"]).cuda() if with_top else None
    torch.cuda.synchronize()  # (the context has a stream of its own)
    s, plain = ctx.simplified_outlines_dev(d_label.data_ptr(), d_top.data_ptr() if with_top else 0, w, h, c["n_labels"], *tol)
    assert s.sxy is None and s.sz is None and s.s_right is None and s.s_flag is None and s.has_z == with_top
    outs = []
    for _ in range(2):  # the emit may be called more than once
        nv = s.n_svertices
        d_xy = torch.full((nv, 2), PATTERN, dtype=torch.int32, device="cuda")
        d_z = torch.full((nv,), PATTERN, dtype=torch.int32, device="cuda") if with_top else None
        d_right = torch.full((nv,), PATTERN, dtype=torch.int32, device="cuda")
        d_flag = torch.full((nv,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.simplified_outlines_emit_dev(d_xy.data_ptr(), d_z.data_ptr() if with_top else 0, d_right.data_ptr(), d_flag.data_ptr())
        outs.append([t.cpu().numpy() if t is not None else None for t in (d_xy, d_z, d_right, d_flag)])
    for a, b in zip(*outs):
        if a is not None:
            assert (a != (0xA5 if a.dtype == np.uint8 else PATTERN)).all() and np.array_equal(a, b)  # every element, twice the same
    s.sxy, s.sz, s.s_right, s.s_flag = outs[0]
    return s, plain


def test_device_pointers(gpu_ctx):
    for name, tol in (("fuzz_1", (1, 1)), ("spiral", (2, 1)), ("fuzz_9", (0, 1))):  # one context: the scratch is reused
        c = NAMED[name]
        plain, want = cases.run_ref(c, tol)
        for with_top in (True, False):
            got, gp = dev_run(gpu_ctx, c, tol, with_top)
            if not with_top:
                got.sz = want.sz
            assert sref.same(got, want) is None, sref.same(got, want)
            assert same_plain(gp, plain) is None


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_error_paths(gpu_ctx):
    import torch
    ctx = gpu_ctx
    c, tol = NAMED["fuzz_5"], (1, 1)
    plain, want = cases.run_ref(c, tol)
    h, w = c["label"].shape
    d_label, d_top = torch.from_numpy(c["label"]).cuda(), torch.from_numpy(c["top"]).cuda()
    nv = want.n_svertices
    d_xy = torch.full((nv, 2), PATTERN, dtype=torch.int32, device="cuda")
    d_z = torch.full((nv,), PATTERN, dtype=torch.int32, device="cuda")
    d_right = torch.full((nv,), PATTERN, dtype=torch.int32, device="cuda")
    d_flag = torch.full((nv,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    emit = lambda h_=None: ctx._L.bs_simple_outlines_emit_dev(h_ or ctx._h, d_xy.data_ptr(), d_z.data_ptr(), d_right.data_ptr(),  # noqa: E731
                                                              d_flag.data_ptr())

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == p).all()) for t, p in ((d_xy, PATTERN), (d_z, PATTERN), (d_right, PATTERN), (d_flag, 0xA5)))

    def raw(**kw):
        a = dict(d_label=d_label.data_ptr(), d_top=d_top.data_ptr(), width=w, height=h, n_labels=c["n_labels"], num=tol[0],
                 den=tol[1])
        a.update(kw)
        out, pl = _lib.SimpleOutlines(), _lib.Outlines()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        C.memset(C.byref(pl), 0x5A, C.sizeof(pl))
        rc = ctx._L.bs_simple_outlines_count_dev(ctx._h, a["d_label"] or None, a["d_top"] or None, a["width"], a["height"],
                                                 a["n_labels"], a["num"], a["den"], C.byref(out), C.byref(pl))
        return rc, out, pl

    def good():
        """a following good call equals the reference"""
        got, gp = dev_run(ctx, c, tol, True)
        assert sref.same(got, want) is None and same_plain(gp, plain) is None

    def failed(rc, out, pl, status):
        assert rc == status
        assert bytes(out) == b"\x5a" * C.sizeof(out) and bytes(pl) == b"\x5a" * C.sizeof(pl)  # the outputs are untouched
        assert emit() == -1 and untouched()  # an emit after a failed count

    # an emit before any count, on a context of its own
    with api.Context(0) as fresh:
        assert emit(fresh._h) == -1
    assert untouched()
    for kw in (dict(den=0), dict(num=-1), dict(den=-4), dict(num=1 << 31), dict(den=1 << 31), dict(width=0), dict(d_label=0),
               dict(n_labels=-1), dict(d_top=d_top.data_ptr() + 4)):
        good()
        failed(*raw(**kw), -1)
    assert b"simplified outlines" in ctx._L.bs_last_error(ctx._h)
    # BS_ERR_RANGE: a label >= n_labels
    good()
    lab = c["label"].copy()
    lab[tuple(np.argwhere(lab >= 0)[0])] = c["n_labels"]
    d_bad = torch.from_numpy(lab).cuda()
    torch.cuda.synchronize()
    failed(*raw(d_label=d_bad.data_ptr()), -2)
    with pytest.raises(api.BsError) as e:  # the host-memory twin reports the same
        ctx.simplified_outlines(lab, c["top"], n_labels=c["n_labels"], num=1, den=1)
    assert e.value.status == -2
    with pytest.raises(api.BsError) as e:
        ctx.simplified_outlines(c["label"], c["top"], n_labels=c["n_labels"], num=1, den=0)
    assert e.value.status == -1
    # d_sz against the count: missing with top
    good()
    assert ctx._L.bs_simple_outlines_emit_dev(ctx._h, d_xy.data_ptr(), None, d_right.data_ptr(), d_flag.data_ptr()) == -1
    assert untouched()
    # the context is as usable as before, for this stage and the plain outlines
    good()
    o = ctx.facet_outlines(c["label"], c["top"], n_labels=c["n_labels"])
    assert orf.same(o, orf.outlines(c["label"], c["top"], c["n_labels"])) is None


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_gabled_scene_roof_polygons(gpu_ctx, tmp_path):
    sc = load_roof_scenes()
    xyz = sc.gabled()
    _, _, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=15))
    fp, b, r, s = gpu_ctx.solid_model(xyz, plane_idx, planes, refit=True)
    rf = gpu_ctx.roof_structure(b.map, r, s)
    h, w = rf.facet.shape
    before = None
    for mm in (0, 100, 200):
        o, plain = gpu_ctx.roof_polygons(rf, s, tolerance_mm=mm)
        num, den = api.simplify_tolerance(mm, s.bin)
        want = sref.simplify(rf.facet, s.top, rf.n_facets, num, den)
        assert sref.same(o, want[1]) is None, sref.same(o, want[1])
        twin_identity(plain, o)
        print("gable: tolerance", mm, "mm: nodes", o.n_nodes, "arcs", o.n_arcs, "rounds", o.rounds, "vertices", plain.n_vertices,
              "->", o.n_svertices)
        assert before is None or o.n_svertices <= before
        before = o.n_svertices
        # Z at every kept vertex = top read from ANY pixel of the facet at that corner
        lab = np.repeat(plain.ring_label, o.s_ring_vertices)
        seen = np.zeros(o.n_svertices, np.int64)
        for (ox, oy), t in (((-1, -1), 3), ((0, -1), 2), ((-1, 0), 1), ((0, 0), 0)):  # the pixel at this offset has the corner as t
            px, py = o.sxy[:, 0] + ox, o.sxy[:, 1] + oy
            ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            ok[ok] = rf.facet[py[ok], px[ok]] == lab[ok]
            assert np.array_equal(s.top[py[ok], px[ok], t], o.sz[ok])
            seen += ok
        assert (seen >= 1).all()
    assert o.n_svertices < plain.n_vertices
    api.write_simple_outlines_obj(o, tmp_path / "polygons.obj", s.bin, origin=(0, 0, 0))
    assert open(tmp_path / "polygons.obj", "rb").read() == cases.brute.obj_text(plain, o, s.bin, num, den, (0, 0, 0))
    with pytest.raises(ValueError):
        gpu_ctx.roof_polygons(api.RoofFacets(**{**vars(rf), "facet": None}), s)
