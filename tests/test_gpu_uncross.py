"""Clean outlines on the device (bs_clean_outlines, bs_clean_outlines_count_dev / _emit_dev; include/bs_api.h) against
the numpy restatement tests/uncross_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_roofs_cpu import load_roof_scenes  # noqa: E402
from test_simplify_cpu import twin_identity  # noqa: E402
from test_uncross_cpu import load_uncross_cases, marked_by_all_pairs  # noqa: E402

cases = load_uncross_cases()
uref, brute, sc = cases.uref, cases.brute, cases.sc
sref = uref.sref
orf = sc.oc.orf

pytestmark = pytest.mark.gpu

NAMED = dict(cases.named_cases())
PLAIN_FIELDS = [f for f in orf.brute.FIELDS if f not in ("xy", "z")]
SIMPLE_FIELDS = [f for f in sref.brute.FIELDS if f not in ("sxy", "sz", "s_right", "s_flag")]


def same_fields(got, want, fields):
    for f in fields:
        if not np.array_equal(np.asarray(getattr(got, f), np.int64), np.asarray(getattr(want, f), np.int64)):
            return f
    return None


def check(ctx, c, tol, cell_log2=0, max_rounds=-1, tops=(True, False)):
    """the host-memory entry point with top and without against the restatement: every array, figure and total"""
    plain, simple, want = uref.clean(c["label"], c["top"], c["n_labels"], *tol, max_rounds=max_rounds, cell_log2=cell_log2)
    for with_top in tops:
        got, gs, gp = ctx.clean_outlines(c["label"], c["top"] if with_top else None, n_labels=c["n_labels"], num=tol[0],
                                         den=tol[1], max_rounds=max_rounds, cell_log2=cell_log2)
        assert got.has_z == with_top and (got.sz is not None) == with_top
        if not with_top:
            got.sz = want.sz
        assert uref.same(got, want, uref.DEVICE_FIELDS) is None, (tol, with_top, uref.same(got, want, uref.DEVICE_FIELDS))
        assert (got.tol_num, got.tol_den, got.max_rounds) == tol + (max_rounds,)
        assert got.cell_log2 == (cell_log2 or uref.DEFAULT_CELL_LOG2)
        assert same_fields(gp, plain, PLAIN_FIELDS) is None and same_fields(gs, simple, SIMPLE_FIELDS) is None
        assert gs.sxy is None and gp.xy is None
        assert np.array_equal(got.ring_label, plain.ring_label) and np.array_equal(got.ring_area2, plain.ring_area2)
    return got, gp


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case(gpu_ctx, name):
    """every named case at every tolerance, at the default cell size"""
    for tol in cases.TOLERANCES:
        check(gpu_ctx, NAMED[name], tol)


@pytest.mark.parametrize("name,tol", cases.CONFLICTING, ids=[f"{n}-{t[0]}" for n, t in cases.CONFLICTING])
def test_conflicting_runs_at_every_cell_size(gpu_ctx, name, tol):
    """one corner pair per cell, many cells, one cell (the tile kernel takes runs of more than 64 entries)"""
    for k in cases.CELL_LOG2:
        got, gp = check(gpu_ctx, NAMED[name], tol, cell_log2=k, tops=(True,))
        assert got.n_marked_first > 0 and not marked_by_all_pairs(gp, got)
        twin_identity(gp, got)
    check(gpu_ctx, NAMED[name], tol, max_rounds=0)
    check(gpu_ctx, NAMED[name], tol, max_rounds=1, cell_log2=30)


@pytest.mark.parametrize("name,tol", cases.CONFLICTING_FUZZ, ids=[f"{n}-{t[0]}" for n, t in cases.CONFLICTING_FUZZ])
def test_conflicting_fuzz_runs(gpu_ctx, name, tol):
    """the facet fuzz cases that conflict, thousands of segments each, at the two smaller cell sizes"""
    for k in cases.CELL_LOG2[:2]:
        got, gp = check(gpu_ctx, NAMED[name], tol, cell_log2=k, tops=(True,))
        assert got.n_marked_first > 0 and got.n_marked_left == 0
    check(gpu_ctx, NAMED[name], tol, max_rounds=0, tops=(True,))


def test_long_segment_walks_its_columns(gpu_ctx):
    """thin_u_400 at cell_log2 = 1: a segment that spans 200 columns of cells"""
    t = {}
    c = sc.thin_u()
    uref.clean(c["label"], c["top"], c["n_labels"], cases.BIG_DEN, cases.BIG_DEN, cell_log2=1, trace=t)
    assert t["max_span"] >= 100
    check(gpu_ctx, c, (cases.BIG_DEN, cases.BIG_DEN), cell_log2=1, tops=(True,))
    check(gpu_ctx, c, (cases.BIG_DEN, cases.BIG_DEN), cell_log2=30, tops=(True,))


def test_noise_crosses_the_entry_sweep(gpu_ctx):
    """470 x 470 of noise that is mostly one label, at (25, 4) and cell_log2 = 1: more entries than one sweep of 1024 x 256
    (420 x 420 stays below), with conflicts to repair (noise of equal shares has none: nearly every node is a junction)"""
    n = 470
    rng = np.random.default_rng(12)
    lab = rng.integers(-1, 3, (n, n)).astype(np.int32)
    lab = np.where(rng.random((n, n)) < 0.8, 0, lab).astype(np.int32)
    c = dict(label=lab, top=rng.integers(-500, 500, (n, n, 4)).astype(np.int32), n_labels=3)
    plain, simple, want = uref.clean(lab, c["top"], 3, 25, 4, cell_log2=1)
    assert want.n_entries > 1024 * 256 and want.n_marked_first > 0 and want.repair_rounds >= 1
    got, gs, gp = gpu_ctx.clean_outlines(lab, c["top"], n_labels=3, num=25, den=4, cell_log2=1)
    assert uref.same(got, want, uref.DEVICE_FIELDS) is None, uref.same(got, want, uref.DEVICE_FIELDS)
    print("noise: segments", want.n_svertices_before, "entries", want.n_entries, "marked", want.n_marked_first, "rounds",
          want.repair_rounds, "forced", want.n_forced, "max cell", want.max_cell_entries)


PATTERN = -0x5A5A5A5B


def test_device_pointers_and_errors(gpu_ctx):
    import torch
    ctx = gpu_ctx
    c, tol = NAMED["finger"], (10 ** 6, 1)
    plain, simple, want = uref.clean(c["label"], c["top"], c["n_labels"], *tol)
    h, w = c["label"].shape
    d_label, d_top = torch.from_numpy(c["label"]).cuda(), torch.from_numpy(c["top"]).cuda()
    nv = want.n_svertices
    d_xy = torch.full((nv, 2), PATTERN, dtype=torch.int32, device="cuda")
    d_z = torch.full((nv,), PATTERN, dtype=torch.int32, device="cuda")
    d_right = torch.full((nv,), PATTERN, dtype=torch.int32, device="cuda")
    d_flag = torch.full((nv,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with api.Context(0) as fresh:  # an emit without a count
        assert fresh._L.bs_clean_outlines_emit_dev(fresh._h, d_xy.data_ptr(), d_z.data_ptr(), d_right.data_ptr(), d_flag.data_ptr()) == -1
    for bad in (-1, 31):  # bad cell_log2: the outputs stay untouched
        out, sm, pl = _lib.CleanOutlines(), _lib.SimpleOutlines(), _lib.Outlines()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        rc = ctx._L.bs_clean_outlines_count_dev(ctx._h, d_label.data_ptr(), d_top.data_ptr(), w, h, c["n_labels"], tol[0], tol[1], -1, bad,
                                                C.byref(out), C.byref(sm), C.byref(pl))
        assert rc == -1 and bytes(out) == b"\x5a" * C.sizeof(out) and b"cell_log2" in ctx._L.bs_last_error(ctx._h)
    with pytest.raises(api.BsError):
        ctx.clean_outlines(c["label"], c["top"], n_labels=c["n_labels"], num=1, den=0)
    got, gs, gp = ctx.clean_outlines_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, c["n_labels"], *tol)
    assert got.sxy is None and got.n_svertices == nv
    # a wrong d_sz: missing with top
    assert ctx._L.bs_clean_outlines_emit_dev(ctx._h, d_xy.data_ptr(), None, d_right.data_ptr(), d_flag.data_ptr()) == -1
    torch.cuda.synchronize()
    assert bool((d_xy == PATTERN).all()) and bool((d_flag == 0xA5).all())
    for _ in range(2):
        ctx.clean_outlines_emit_dev(d_xy.data_ptr(), d_z.data_ptr(), d_right.data_ptr(), d_flag.data_ptr())
    got.sxy, got.sz, got.s_right, got.s_flag = (t.cpu().numpy() for t in (d_xy, d_z, d_right, d_flag))
    assert uref.same(got, want, uref.DEVICE_FIELDS) is None
    # simple and plain equal what bs_simple_outlines returns on the same input
    s2, p2 = ctx.simplified_outlines(c["label"], c["top"], n_labels=c["n_labels"], num=tol[0], den=tol[1])
    assert same_fields(gs, s2, SIMPLE_FIELDS) is None and same_fields(gp, p2, PLAIN_FIELDS) is None


def test_writer_against_the_reference_text(gpu_ctx, tmp_path):
    c, tol = NAMED["finger"], (10 ** 6, 1)
    got, _, gp = gpu_ctx.clean_outlines(c["label"], c["top"], n_labels=c["n_labels"], num=tol[0], den=tol[1])
    api.write_clean_outlines_obj(got, tmp_path / "c.obj", 25, origin=(1000, -2000, 30))
    text = open(tmp_path / "c.obj", "rb").read()
    assert text == brute.obj_text(gp, got, 25, tol[0], tol[1], (1000, -2000, 30))
    assert text.startswith(b"# clean outlines: 3 labels, 4 rings, 26 vertices, tol2 1000000/1, repair_rounds 3, n_forced 10\n")


def test_gabled_scene_clean_roof_polygons(gpu_ctx):
    sc_ = load_roof_scenes()
    xyz = sc_.gabled()
    _, _, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=15))
    fp, b, r, s = gpu_ctx.solid_model(xyz, plane_idx, planes, refit=True)
    rf = gpu_ctx.roof_structure(b.map, r, s)
    for mm in (100, 400):
        o, plain = gpu_ctx.roof_polygons(rf, s, tolerance_mm=mm, clean=True)
        num, den = api.simplify_tolerance(mm, s.bin)
        _, _, want = uref.clean(rf.facet, s.top, rf.n_facets, num, den)
        assert uref.same(o, want, uref.DEVICE_FIELDS) is None, uref.same(o, want, uref.DEVICE_FIELDS)
        twin_identity(plain, o)
        assert o.n_marked_left == 0
        before, _ = gpu_ctx.roof_polygons(rf, s, tolerance_mm=mm)  # the default keeps its behaviour and return value
        assert isinstance(before, api.SimpleOutlines) and not isinstance(before, api.CleanOutlines)
        assert before.n_svertices == o.n_svertices_before
        print("gable: tolerance", mm, "mm: marked", o.n_marked_first, "rounds", o.repair_rounds, "forced", o.n_forced)
