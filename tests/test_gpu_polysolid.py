"""Polygon solids on the device (bs_poly_solids, bs_poly_solids_count_dev / _emit_dev; include/bs_api.h) against the numpy
restatement tests/polysolid_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_roofs_cpu import load_roof_scenes  # noqa: E402
from test_polysolid_cpu import BY_NAME, OWN, check_promises, load_polysolid_cases, ref, upstream  # noqa: E402

cases = load_polysolid_cases()
pref, brute, tref, tbrute, uref = cases.pref, cases.brute, cases.tref, cases.tbrute, cases.uref

pytestmark = pytest.mark.gpu
BIN = cases.BIN


def check(ctx, name, tol, kind, base):
    """the host-memory entry point against the restatement over the restated stages before: every array and figure"""
    c = BY_NAME[name][0]
    want, _, lb, nb = ref(name, tol, kind, base)
    plain, clean, tri = upstream(name, tol)
    got, gt, gc, gs, gp = ctx.poly_solids(c["label"], c["top"], lb, n_labels=c["n_labels"], n_buildings=nb, num=tol[0], den=tol[1],
                                          bin=BIN, base_z=base)
    assert pref.same(got, want) is None, (name, tol, kind, base, pref.same(got, want))
    assert (got.n_buildings, got.n_labels, got.bin, got.base_z, got.fig_cap) == (nb, c["n_labels"], BIN, base, pref.FIG_CAP)
    assert tref.same(gt, tri) is None and np.array_equal(gc.sxy, clean.sxy) and np.array_equal(gc.sz, clean.sz)
    assert gs.sxy is None and gp.xy is None and np.array_equal(gp.label_ring_offset, plain.label_ring_offset)
    return got


def against_own_upstream(ctx, label, top, lb, nb, base, tol=(0, 1), n_labels=None):
    """the device against the restatement of this stage over the device's own clean outlines and triangles (the stages before
    have their own tests): for images too large for the restatements of the whole chain"""
    got, gt, gc, _, gp = ctx.poly_solids(label, top, lb, n_labels=n_labels, n_buildings=nb, num=tol[0], den=tol[1], bin=BIN, base_z=base)
    want = pref.poly_solids(gp, gc, gt, lb, nb, BIN, base)
    assert pref.same(got, want) is None, pref.same(got, want)
    return got, gt, gc


def variants(name):
    """an upstream run of the named cases with both building tables, base_z alternating; a shape of this stage with all of
    its own"""
    runs = BY_NAME[name][1]
    if name in OWN:
        return runs
    tols = sorted({r[0] for r in runs}, key=[r[0] for r in runs].index)
    return [(tol, kind, cases.BASES[(i + j) % 2]) for i, tol in enumerate(tols) for j, kind in enumerate(cases.TABLES)]


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_case(gpu_ctx, name):
    """every named case at every tolerance of its own with both building tables; the wall shapes, the other sides of a wall,
    the corner of four labels, pinched, nested, two_outers, the label without a ring and the building counts round the cap
    of the figure tables are names of this list"""
    for tol, kind, base in variants(name):
        check(gpu_ctx, name, tol, kind, base)


def test_shapes_on_the_device(gpu_ctx):
    """what the shapes are for, read from the device's result"""
    s = check(gpu_ctx, "wall_8", (0, 1), "one", -1000)
    assert s.max_wall_vertices_all == 8
    assert check(gpu_ctx, "wall_crossing", (0, 1), "one", -1000).n_crossing_walls == 1
    assert check(gpu_ctx, "wall_below_base", (0, 1), "one", 1000).total_volume6 < 0
    assert check(gpu_ctx, "sieve_24", (0, 1), "one", -1000).n_wall_faces >= 4 * 64  # (64 courtyards of one pixel)
    for n in (1023, 1024, 1025, 5000):
        s = check(gpu_ctx, f"strip_{n}", (0, 1), "each", -1000)
        assert (s.wall_faces == 4).all() and (s.vertices == 8).all() and len(s.volume6) == n
        check_promises(s, BIN)


def test_no_labelled_pixel(gpu_ctx):
    """an empty mesh; the emit writes face_offset[0] alone"""
    import torch
    s = check(gpu_ctx, "no_label_pixel", (0, 1), "mod3", 0)
    assert (s.n_vertices, s.n_faces, s.n_indices) == (0, 0, 0) and s.face_offset.tolist() == [0] and s.vertex.shape == (0, 4)
    lab = torch.full((3, 4), -1, dtype=torch.int32, device="cuda")
    top = torch.zeros((3, 4, 4), dtype=torch.int32, device="cuda")
    lb = torch.zeros(2, dtype=torch.int32, device="cuda")
    off = torch.full((4,), PATTERN, dtype=torch.int32, device="cuda")
    got = gpu_ctx.poly_solids_dev(lab.data_ptr(), top.data_ptr(), 4, 3, 2, lb.data_ptr(), 1)[0]
    assert got.n_faces == 0 and got.vertex is None
    gpu_ctx.poly_solids_emit_dev(0, off.data_ptr(), 0, 0, 0)
    assert off.cpu().tolist() == [0, PATTERN, PATTERN, PATTERN]


def test_open_building_beside_closed_ones(gpu_ctx):
    """random_0 at (10^6, 1) with label % 3: label 0 is NO_BRIDGE, building 0 emits nothing, buildings 1 and 2 are whole"""
    (name, tol, l), = cases.tc.NO_BRIDGE_RUNS
    s = check(gpu_ctx, name, tol, "mod3", -1000)
    assert s.status.tolist() == [1, 0, 0] and s.n_open_buildings == 1 and s.vertices[0] == 0 and s.faces[0] == 0
    assert not (s.face_building == 0).any() and not (s.vertex[:, 3] == 0).any() and s.faces[1] > 0
    check_promises(s, BIN)
    s = check(gpu_ctx, name, tol, "one", 0)
    assert s.n_faces == 0 and s.n_vertices == 0 and s.status.tolist() == [1]


def test_noise_crosses_every_sweep_and_tile(gpu_ctx):
    """random labels per pixel, 400 x 400: the grid-stride passes take 1024 workgroups of 256, so one sweep is 262 144 items
    -- the clean vertices (about 600 000), the vertex entries (twice that) and the triangles (about 300 000) all exceed it,
    and with it one tile of the radix sorts and the scans (a few thousand items a tile).  Buildings: 3000 by label % 3000,
    beyond the cap of the figure tables."""
    rng = np.random.default_rng(77)
    nl, nb = 50000, 3000
    lab = rng.integers(-1, nl, (400, 400)).astype(np.int32)
    top = rng.integers(-500, 500, (400, 400, 4)).astype(np.int32)
    lb = (np.arange(nl) % nb).astype(np.int32)
    s, t, c = against_own_upstream(gpu_ctx, lab, top, lb, nb, 0, n_labels=nl)
    print("noise: clean vertices", c.n_svertices, "triangles", t.n_triangles, "mesh vertices", s.n_vertices, "faces", s.n_faces,
          "walls", s.n_wall_faces, "crossing", s.n_crossing_walls, "open", s.n_open_buildings, s.info)
    assert c.n_svertices > 262144 and t.n_triangles > 262144 and s.n_open_buildings == 0
    assert s.n_wall_faces > 262144 and s.wall_faces[pref.FIG_CAP:].sum() > 0


def test_blobs_keep_waves_inside_one_building(gpu_ctx):
    """large blobs at a tolerance: long runs of clean vertices of one building (the register path of the figures)"""
    rng = np.random.default_rng(78)
    coarse = rng.integers(-1, 40, (12, 16)).astype(np.int32)
    lab = np.kron(coarse, np.ones((25, 25), np.int32)).astype(np.int32)
    lab[rng.random(lab.shape) < 0.02] = -1
    top = rng.integers(-500, 500, lab.shape + (4,)).astype(np.int32)
    lb = (np.arange(40) % 7).astype(np.int32)
    for tol in ((0, 1), (4, 1)):
        s, t, c = against_own_upstream(gpu_ctx, lab, top, lb, 7, -1000, tol, n_labels=40)
        assert c.n_svertices > 64 * 40


PATTERN = -0x5A5A5A5B


def mesh_buffers(torch, s):
    return [torch.full(shape, PATTERN if dt != torch.uint8 else 0xA5, dtype=dt, device="cuda")
            for shape, dt in (((s.n_vertices, 4), torch.int32), ((s.n_faces + 1,), torch.int32), ((s.n_indices,), torch.int32),
                              ((s.n_faces,), torch.int32), ((s.n_faces,), torch.uint8))]


def test_device_pointers_and_errors(gpu_ctx):
    import torch
    ctx = gpu_ctx
    name, tol, kind, base = "nested", (0, 1), "mod3", 0
    c = BY_NAME[name][0]
    want, _, lb, nb = ref(name, tol, kind, base)
    h, w = c["label"].shape
    nl = c["n_labels"]
    clean_z_max = upstream(name, tol)[1].sz.max()
    d_label, d_top, d_lb = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c["label"], c["top"], lb))
    bufs = mesh_buffers(torch, want)
    ptrs = [b.data_ptr() for b in bufs]
    torch.cuda.synchronize()
    with api.Context(0) as fresh:  # an emit without a count
        assert fresh._L.bs_poly_solids_emit_dev(fresh._h, *ptrs) == -1
        assert b"without a successful count" in fresh._L.bs_last_error(fresh._h)

    def count(out, top=d_top.data_ptr(), table=d_lb.data_ptr(), n_buildings=nb, bin=BIN, base_z=base, tri=None):
        return ctx._L.bs_poly_solids_count_dev(ctx._h, d_label.data_ptr(), top, w, h, nl, tol[0], tol[1], 0, table, n_buildings, bin,
                                               base_z, out, tri, None, None, None)

    def untouched(**kw):
        out, tri = _lib.PolySolids(), _lib.OutlineTriangles()
        C.memset(C.byref(out), 0x5A, C.sizeof(out))
        C.memset(C.byref(tri), 0x5A, C.sizeof(tri))
        rc = count(C.byref(out), tri=C.byref(tri), **kw)
        msg = ctx._L.bs_last_error(ctx._h)
        assert bytes(out) == b"\x5a" * C.sizeof(out) and bytes(tri) == b"\x5a" * C.sizeof(tri)
        assert ctx._L.bs_poly_solids_emit_dev(ctx._h, *ptrs) == -1  # a failed count leaves nothing to emit
        return rc, msg

    assert count(None) == -1
    rc, msg = untouched(top=None)  # BS_ERR_INVALID
    assert rc == -1 and b"no top image" in msg
    assert untouched(bin=0)[0] == -1 and untouched(n_buildings=-1)[0] == -1 and untouched(table=None)[0] == -1
    rc, msg = untouched(n_buildings=nb - 1)  # BS_ERR_RANGE: a label_building value equal to n_buildings
    assert rc == -2 and b"label_building" in msg
    rc, msg = untouched(base_z=int(clean_z_max) - (1 << 24))  # BS_ERR_RANGE: a top 2^24 above base_z
    assert rc == -2 and b"2^24" in msg
    assert _lib.STATUS[-2] == "BS_ERR_RANGE" and _lib.STATUS[-1] == "BS_ERR_INVALID"
    with pytest.raises(api.BsError):
        ctx.poly_solids(c["label"], c["top"], lb, n_labels=nl, n_buildings=nb - 1)
    torch.cuda.synchronize()
    assert all(bool((b == (PATTERN if b.dtype != torch.uint8 else 0xA5)).all()) for b in bufs)
    # a following valid call succeeds; the count and the emit equal the host-memory entry point
    got, gt, gc, gs, gp = ctx.poly_solids_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, nl, d_lb.data_ptr(), nb, *tol, bin=BIN,
                                              base_z=base)
    assert got.vertex is None and gt.tri is None and gc.sxy is None
    assert (got.n_vertices, got.n_faces, got.n_indices) == (want.n_vertices, want.n_faces, want.n_indices)
    assert ctx._L.bs_poly_solids_emit_dev(ctx._h, ptrs[0], None, *ptrs[2:]) == -1  # a missing buffer
    first = None
    for _ in range(2):  # the emit twice: the same bytes
        for b in bufs:
            b.fill_(PATTERN if b.dtype != torch.uint8 else 0xA5)
        ctx.poly_solids_emit_dev(*ptrs)
        b = b"".join(x.cpu().numpy().tobytes() for x in bufs)
        assert first is None or b == first
        first = b
    got.vertex, got.face_offset, got.face_index, got.face_building, got.face_kind = (x.cpu().numpy() for x in bufs)
    assert pref.same(got, want) is None, pref.same(got, want)
    host = ctx.poly_solids(c["label"], c["top"], lb, n_labels=nl, n_buildings=nb, num=tol[0], den=tol[1], bin=BIN, base_z=base)[0]
    assert pref.same(got, host) is None
    # the triangles of the same count are still there for their own emit; a clean count afterwards ends the emit's validity
    ctx.poly_solids_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, nl, d_lb.data_ptr(), nb, *tol, bin=BIN, base_z=base)
    d_tri = torch.zeros((upstream(name, tol)[2].n_triangles, 3), dtype=torch.int32, device="cuda")
    ctx.outline_triangles_emit_dev(d_tri.data_ptr())
    assert np.array_equal(d_tri.cpu().numpy(), upstream(name, tol)[2].tri)
    ctx.clean_outlines_dev(d_label.data_ptr(), d_top.data_ptr(), w, h, nl, *tol)
    assert ctx._L.bs_poly_solids_emit_dev(ctx._h, *ptrs) == -1


def test_writer_against_the_reference_text(gpu_ctx, tmp_path):
    for name, tol, kind, base in (("nested", (0, 1), "mod3", -1000), ("random_0", (10 ** 6, 1), "mod3", 0)):
        s = check(gpu_ctx, name, tol, kind, base)
        api.write_solids_obj(s, tmp_path / "p.obj", origin=(1000, -2000, 30))
        assert open(tmp_path / "p.obj", "rb").read() == brute.obj_text(ref(name, tol, kind, base)[0], (1000, -2000, 30))


def test_building_model(gpu_ctx):
    """building_model on a facet fuzz case and on the gabled scene through solid_model -> roof_structure equals the direct
    call and the restatement"""
    ctx = gpu_ctx
    fz = cases.sc.fc.fuzz_case(2)
    rf = ctx.roof_facets(fz["bmap"], fz["roof"], fz["top"], n_buildings=fz["n_buildings"], n_planes=fz["n_planes"])
    sol = SimpleNamespace(top=fz["top"], bin=fz["bin"], base_z=-1000, n_buildings=fz["n_buildings"])
    todo = [(rf, sol, (0, 3 * fz["bin"]))]
    xyz = load_roof_scenes().gabled()
    _, _, plane_idx, planes = ctx.segment(xyz, api.default_params(k=15))
    fp, b, r, s = ctx.solid_model(xyz, plane_idx, planes, refit=True)
    todo.append((ctx.roof_structure(b.map, r, s), s, (0, 400)))
    for rf, sol, tolerances in todo:
        for mm in tolerances:
            p, t, o, plain = ctx.building_model(rf, sol, tolerance_mm=mm)
            num, den = api.simplify_tolerance(mm, sol.bin)
            d = ctx.poly_solids(rf.facet, sol.top, rf.facet_building, n_labels=rf.n_facets, n_buildings=sol.n_buildings, num=num,
                                den=den, bin=sol.bin, base_z=sol.base_z)[0]
            assert pref.same(p, d) is None
            wp, _, wc = uref.clean(rf.facet, sol.top, rf.n_facets, num, den)
            want = pref.poly_solids(wp, wc, tref.triangulate(wp, wc), rf.facet_building, sol.n_buildings, sol.bin, sol.base_z)
            assert pref.same(p, want) is None, pref.same(p, want)
            check_promises(p, sol.bin)
            print("building model: tolerance", mm, "mm: vertices", p.n_vertices, "faces", p.n_faces, "walls", p.n_wall_faces,
                  "crossing", p.n_crossing_walls, "open", p.n_open_buildings)
