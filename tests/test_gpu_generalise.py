"""Roof generalisation on the device (bs_roof_generalise, bs_roof_generalise_dev; include/bs_api.h) against the numpy
restatement tests/generalise_ref.  Everything is an exact integer: every comparison is ==."""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_generalise_cpu import idempotent, identities, load_generalise_cases  # noqa: E402
from test_roofs_cpu import load_roof_scenes  # noqa: E402

cases = load_generalise_cases()
gr, fr, sr, sc = cases.gr, cases.fr, cases.sr, cases.sc

pytestmark = pytest.mark.gpu
SHAPES = cases.named_shapes()
TABLES = ("normal", "center", "z_min", "z_max", "bin", "base_z", "flat")


def roofs_of(c):
    return SimpleNamespace(roof=c["roof"], normal=c["normal"], center=c["center"], z_min=c["z_min"], z_max=c["z_max"], bin=c["bin"])


def run(ctx, c):
    return ctx.generalise_roofs(c["bmap"], roofs_of(c), base_z=c["base_z"], flat=c["flat"], **c["params"])


def check(ctx, c, want=None):
    got, want = run(ctx, c), cases.run_ref(c) if want is None else want
    assert gr.same(got, want) is None, (gr.same(got, want), getattr(got, gr.same(got, want)), getattr(want, gr.same(got, want)))
    h, w = c["bmap"].shape
    assert (got.width, got.image_height, got.n_buildings, got.n_planes) == (w, h, c["n_buildings"], len(c["z_min"]))
    assert np.array_equal(got.roofs.roof, got.roof) and np.array_equal(got.roofs.pixels, got.plane_pixels_out[1:])
    return got


def to_dev(c):
    import torch
    d_map, d_roof = (torch.from_numpy(np.ascontiguousarray(c[k], np.int32)).cuda() for k in ("bmap", "roof"))
    torch.cuda.synchronize()
    return d_map, d_roof


def dev_run(ctx, c, d_map, d_roof, d_out):
    h, w = c["bmap"].shape
    return ctx.generalise_roofs_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, *[c[k] for k in TABLES], d_out.data_ptr(),
                                    **c["params"])


# ---- shapes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_named_shape(gpu_ctx, name):
    """the minimal images, the islands, the length ties, the two small facets, the touching buildings, the diagonal, the
    strips, the coplanar pair with and without merge_flat, the gable and the step (what each must do is asserted from the
    reference in tests/test_generalise_cpu.py::test_named_shapes_do_what_they_are_named_for)"""
    got = check(gpu_ctx, SHAPES[name])
    identities(SHAPES[name], got)


def test_no_plane_and_no_building(gpu_ctx):
    c = sc.make(np.zeros((2, 3)), np.zeros((2, 3)), 1, np.zeros((0, 3)), np.zeros((0, 3)), [], [], 10, 0, [50])
    c["params"] = cases.params(min_pixels=100, merge_flat=True)
    got = check(gpu_ctx, c)
    assert got.rounds == 0 and got.plane_pixels_out.tolist() == [6] and got.n_facets_out == 1
    c = cases._shape(np.full((3, 4), -1), np.zeros((3, 4)), nb=0, min_pixels=3)
    got = check(gpu_ctx, c)
    assert got.rounds == 0 and got.n_facets_in == 0 and got.eval_facets.tolist() == [0] and len(got.building_facets_in) == 0


@pytest.mark.parametrize("n", [65, 257, 4097])
def test_chain_lengths(gpu_ctx, n):
    """chains of 64, 256 and 4096 links ending at pixel 0: across a wave, a workgroup and several workgroups of the pointer
    doubling, which takes 7, 9 and 13 rounds"""
    got = check(gpu_ctx, cases.strip(n))
    assert got.eval_longest_chain.tolist() == [n - 1, 0] and got.eval_movers.tolist() == [n - 1, 0]
    assert got.rounds == 1 and (got.roof == 1).all() and got.n_facets_out == 1


# ---- fuzz ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(cases.N_FUZZ))
def test_fuzz(gpu_ctx, seed):
    c = cases.fuzz_case(seed)
    got = check(gpu_ctx, c)
    identities(c, got)
    idempotent(c, got, lambda again: run(gpu_ctx, again))


def test_waiting_facet(gpu_ctx):
    """a small facet whose roofed neighbours all rank lower stays in round 1 and moves later"""
    c = cases.fuzz_case(cases.SEED_WAITS)
    want = cases.run_ref(c)
    assert "waits_then_moves" in cases.regimes(c, want) and want.rounds >= 2
    check(gpu_ctx, c, want)


def test_three_rounds_and_the_round_cap(gpu_ctx):
    c = cases.fuzz_case(cases.SEED_THREE_ROUNDS)
    want = cases.run_ref(c)
    assert want.rounds >= 3 and want.converged == 1
    check(gpu_ctx, c, want)
    # max_rounds = 1: one round applied, the second evaluation still has movers
    capped = cases.with_params(c, max_rounds=1)
    want1 = cases.run_ref(capped)
    assert want1.rounds == 1 and want1.converged == 0 and want1.eval_movers[-1] > 0
    check(gpu_ctx, capped, want1)
    # max_rounds = 0 only reports: the image untouched, the figures of the first evaluation
    got = check(gpu_ctx, cases.with_params(c, max_rounds=0))
    assert got.rounds == 0 and got.converged == 0 and np.array_equal(got.roof, c["roof"]) and got.pixels_changed == 0
    assert got.eval_movers.tolist() == [want.eval_movers[0]] and got.n_facets_out == got.n_facets_in == want.n_facets_in


def test_edge_flat_only_after_a_round(gpu_ctx):
    """a FLAT merge in a later evaluation over pixel edges that lay on an edge of another kind in the first: the applied
    rounds changed the tops"""
    c = cases.fuzz_case(cases.SEED_FLAT_LATER)
    want = cases.run_ref(c)
    assert "flat_only_later" in cases.regimes(c, want)
    check(gpu_ctx, c, want)


def test_min_pixels_one_returns_the_input(gpu_ctx):
    for mp in (0, 1):
        c = cases.with_params(cases.fuzz_case(1), min_pixels=mp, merge_flat=False)
        got = check(gpu_ctx, c)
        assert got.rounds == 0 and got.converged == 1 and np.array_equal(got.roof, c["roof"])


# ---- sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", cases.SIZES)
def test_image_sizes(gpu_ctx, w, h):
    """1, 63, 64, 65 and 129 in both orientations on blob cases"""
    c = cases.blob_case(w, h, seed=w * 1000 + h)
    got = check(gpu_ctx, c)
    identities(c, got)


@pytest.mark.parametrize("w,h", [(65, 17), (17, 65)])
def test_facets_across_tile_seams(gpu_ctx, w, h):
    """one facet over every seam of the labelling tiles with single pixels of another plane on both sides of the seams: all
    of them join it"""
    roof = np.ones((h, w), np.int64)
    roof[::3, 63 % w::4] = 2
    roof[15 % h::7, ::5] = 2
    c = cases._shape(np.zeros((h, w)), roof, min_pixels=4)
    got = check(gpu_ctx, c)
    assert (got.roof == 1).all() and got.n_facets_out == 1 and got.rounds >= 1


def test_large_checkerboard(gpu_ctx):
    """1025 x 1027 pixels, every pixel a facet: more facets and edges than one sweep of the grid-stride passes (4096
    workgroups of 256).  By the tie rule every pixel chains north, and in row 0 west, to pixel 0: one plane after one
    round.  The closed form is asserted; the restatement is not run (its np.unique over two million border edges takes
    longer than a test may)."""
    w, h = 1025, 1027
    assert w * h > 4096 * 256
    c = cases.checkerboard(w, h)
    got = run(gpu_ctx, c)
    n = w * h
    assert (got.rounds, got.converged) == (1, 1) and (got.roof == 1).all()
    assert got.eval_facets.tolist() == [n, 1] and got.eval_movers.tolist() == [n - 1, 0]
    assert got.eval_movers_small.tolist() == [n - 1, 0] and got.eval_movers_flat.tolist() == [0, 0]
    assert got.eval_longest_chain.tolist() == [(w - 1) + (h - 1), 0]
    assert (got.n_edges_in, got.n_edges_out) == (h * (w - 1) + w * (h - 1), 0)
    assert (got.n_flat_in, got.n_small_in, got.n_small_out) == (got.n_edges_in, n, 0)  # 100 mm apart: below step_tol
    assert got.plane_pixels_in.tolist() == [0, (n + 1) // 2, n // 2] and got.plane_pixels_out.tolist() == [0, n, 0]
    assert got.pixels_changed == n // 2 and got.building_sum_abs_dtop.tolist() == [4 * 100 * (n // 2)]
    assert got.building_max_abs_dtop.tolist() == [100] and got.building_facets_in.tolist() == [n]


@pytest.mark.parametrize("d", [-1, 0, 1])
def test_figure_caps(gpu_ctx, d):
    """buildings and planes one below, at and one above the caps of the LDS tables of the figures pass"""
    c = cases.caps_case(cases.FIG_CAP + d, cases.PLANE_CAP + d)
    assert c["bmap"].max() == cases.FIG_CAP + d - 1 and c["roof"].max() == cases.PLANE_CAP + d
    got = check(gpu_ctx, c)
    assert (got.building_pixels_changed == 1).all() and (got.building_facets_out == 1).all()


# ---- device pointers ---------------------------------------------------------------------------------------------------------
def test_device_pointers_and_in_place(gpu_ctx):
    import torch
    for seed in (cases.SEED_THREE_ROUNDS, 2):  # twice on one context: the scratch is reused
        c = cases.fuzz_case(seed)
        want = cases.run_ref(c)
        d_map, d_roof = to_dev(c)
        d_out = torch.full(c["roof"].shape, -7, dtype=torch.int32, device="cuda")
        got = dev_run(gpu_ctx, c, d_map, d_roof, d_out)
        torch.cuda.synchronize()
        got.roof = d_out.cpu().numpy()
        assert gr.same(got, want) is None, gr.same(got, want)
        assert np.array_equal(d_roof.cpu().numpy(), c["roof"]) and np.array_equal(d_map.cpu().numpy(), c["bmap"])
        # d_roof_out == d_roof
        got = dev_run(gpu_ctx, c, d_map, d_roof, d_roof)
        torch.cuda.synchronize()
        got.roof = d_roof.cpu().numpy()
        assert gr.same(got, want) is None, gr.same(got, want)


# ---- errors ----------------------------------------------------------------------------------------------------------------
def raw(ctx, c, dev, **kw):
    """bs_roof_generalise_dev on the device pointers dev = (d_map, d_roof, d_out), single arguments replaced by kw: (status, the struct, filled with a pattern before)"""
    h, w = c["bmap"].shape
    a = dict(d_map=dev[0], d_roof=dev[1], d_out=dev[2], width=w, height=h, n_buildings=c["n_buildings"], n_planes=len(c["z_min"]),
             bin=c["bin"], out=True, params=True, normal=True, flat=True, **c["params"])
    a.update(kw)
    tabs = api._solid_tables(c["normal"], c["center"], c["z_min"], c["z_max"])
    flat = np.ascontiguousarray(c["flat"], np.int32)
    par = _lib.RoofGeneraliseParams(a["min_pixels"], int(a["merge_flat"]), a["step_tol"], a["bend_tol"], a["max_rounds"])
    out = _lib.RoofGeneralise()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    rc = ctx._L.bs_roof_generalise_dev(ctx._h, a["d_map"] or None, a["d_roof"] or None, a["width"], a["height"], a["n_buildings"],
                                       a["n_planes"], tabs[0].ctypes.data if a["normal"] else None,
                                       *[t.ctypes.data for t in tabs[1:]], a["bin"], c["base_z"],
                                       flat.ctypes.data if a["flat"] else None, C.byref(par) if a["params"] else None,
                                       a["d_out"] or None, C.byref(out) if a["out"] else None)
    return rc, out


def test_error_paths(gpu_ctx):
    import torch
    ctx = gpu_ctx
    c = cases.fuzz_case(3)
    assert (c["bmap"] < 0).any() and c["n_buildings"] > 0
    want = cases.run_ref(c)
    d_map, d_roof = to_dev(c)
    d_out = torch.full(c["roof"].shape, -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs = (d_map.data_ptr(), d_roof.data_ptr(), d_out.data_ptr())

    def untouched(out):
        torch.cuda.synchronize()
        return bool((d_out == -7).all()) and bytes(out) == b"\x5a" * C.sizeof(out)

    # BS_ERR_INVALID: the checks of the solids and the facets, and a negative parameter
    for kw in (dict(d_map=0), dict(d_roof=0), dict(d_out=0), dict(out=False), dict(params=False), dict(normal=False),
               dict(flat=False), dict(width=0), dict(height=0), dict(width=-3), dict(height=-1),
               dict(width=1 << 15, height=1 << 15), dict(n_buildings=-1), dict(n_planes=-1), dict(bin=0), dict(min_pixels=-1),
               dict(merge_flat=-1), dict(step_tol=-1), dict(bend_tol=-1), dict(max_rounds=-1)):
        rc, out = raw(ctx, c, ptrs, **kw)
        assert rc == -1, kw
        assert untouched(out), kw
    assert b"roof generalise" in ctx._L.bs_last_error(ctx._h)
    # BS_ERR_RANGE: a map value >= n_buildings, a roof value > n_planes, a roof > 0 outside every building
    inside, outside = np.argwhere(c["bmap"] >= 0)[0], np.argwhere(c["bmap"] < 0)[0]
    for what in ("map", "roof", "roof_outside"):
        m, r = c["bmap"].copy(), c["roof"].copy()
        if what == "map":
            m[tuple(inside)] = c["n_buildings"]
        elif what == "roof":
            r[tuple(inside)] = len(c["z_min"]) + 1
        else:
            r[tuple(outside)] = 1
        dm, dr = torch.from_numpy(m).cuda(), torch.from_numpy(r).cuda()
        torch.cuda.synchronize()
        rc, out = raw(ctx, c, (dm.data_ptr(), dr.data_ptr(), ptrs[2]))
        assert rc == -2 and untouched(out), what
        bad = dict(c, bmap=m, roof=r)
        with pytest.raises(api.BsError) as e:  # the host-memory twin reports the same
            run(ctx, bad)
        assert e.value.status == -2
    # a valid call afterwards: the context is as usable as before
    rc, out = raw(ctx, c, ptrs)
    assert rc == 0
    got = api._take_roof_generalise(ctx._L, out, d_out.cpu().numpy())
    assert gr.same(got, want) is None, gr.same(got, want)
    # the free accepts a zeroed struct
    z = _lib.RoofGeneralise()
    ctx._L.bs_roof_generalise_free(C.byref(z))


# ---- the other stages' state -------------------------------------------------------------------------------------------------
def test_leaves_other_stages_state(gpu_ctx):
    """solids_dev -> generalise_roofs_dev -> solids_emit_dev gives the mesh it gives without the call in between; the same
    for the facet outlines' count and emit, and roof_facets_dev returns what it returned"""
    import torch
    ctx = gpu_ctx
    c = cases.fuzz_case(6)
    g = cases.with_params(cases.fuzz_case(7), min_pixels=9, merge_flat=True)  # another image, of another size
    assert g["bmap"].shape != c["bmap"].shape and cases.run_ref(g).rounds >= 1
    h, w = c["bmap"].shape
    d_map, d_roof = to_dev(c)
    g_map, g_roof = to_dev(g)
    d_top = torch.zeros((h, w, 4), dtype=torch.int32, device="cuda")
    d_facet = torch.zeros((h, w), dtype=torch.int32, device="cuda")

    def between():
        dev_run(ctx, g, g_map, g_roof, g_roof.clone())

    def solids(disturb):
        s = ctx.solids_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, *[c[k] for k in TABLES], d_top=d_top.data_ptr())
        if disturb:
            between()
        i32 = dict(dtype=torch.int32, device="cuda")
        v, off, idx = torch.zeros((max(s.n_vertices, 1), 4), **i32), torch.zeros(s.n_faces + 1, **i32), torch.zeros(max(s.n_indices, 1), **i32)
        fb, kind = torch.zeros(max(s.n_faces, 1), **i32), torch.zeros(max(s.n_faces, 1), dtype=torch.uint8, device="cuda")
        ctx.solids_emit_dev(v.data_ptr(), off.data_ptr(), idx.data_ptr(), fb.data_ptr(), kind.data_ptr())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (v, off, idx, fb, kind)]

    a, b = solids(False), solids(True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a[0]) > 8

    npl = len(c["z_min"])
    f1 = ctx.roof_facets_dev(d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr(), w, h, c["n_buildings"], npl, d_facet.data_ptr())
    img1 = d_facet.cpu().numpy()
    between()
    f2 = ctx.roof_facets_dev(d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr(), w, h, c["n_buildings"], npl, d_facet.data_ptr())
    f1.facet, f2.facet = img1, d_facet.cpu().numpy()
    assert fr.same(f1, f2) is None and f1.n_facets > 1

    def outlines(disturb):
        o = ctx.facet_outlines_dev(d_facet.data_ptr(), d_top.data_ptr(), w, h, f1.n_facets)
        if disturb:
            between()
        xy = torch.zeros((max(o.n_vertices, 1), 2), dtype=torch.int32, device="cuda")
        z = torch.zeros(max(o.n_vertices, 1), dtype=torch.int32, device="cuda")
        ctx.facet_outlines_emit_dev(xy.data_ptr(), z.data_ptr())
        torch.cuda.synchronize()
        return xy.cpu().numpy(), z.cpu().numpy()

    a, b = outlines(False), outlines(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and len(a[0]) > 8


# ---- through the chain -----------------------------------------------------------------------------------------------------
def test_gabled_scene_through_the_chain(gpu_ctx):
    """the gabled scene with seeded speckle in the roof image: after the generalisation the gabled house has its two slopes
    again, the result runs through solids -> facets -> clean outlines -> triangles -> polygon solids and equals their
    references, every building is closed, and the model has fewer vertices than without the stage"""
    from test_polysolid_cpu import check_promises, load_polysolid_cases
    pc = load_polysolid_cases()
    pref, tref, uref = pc.pref, pc.tref, pc.uref
    ctx = gpu_ctx
    scn = load_roof_scenes()
    xyz = scn.gabled()
    _, _, plane_idx, planes = ctx.segment(xyz, api.default_params(k=15))
    fp, b, r, s0 = ctx.solid_model(xyz, plane_idx, planes, refit=True)
    row, cols = scn.gable_pixels()
    house = int(b.map[row, cols[0]])
    pw, pe = int(r.roof[row, cols[0]]), int(r.roof[row, cols[-1]])
    assert house >= 0 and pw > 0 and pe > 0 and pw != pe
    # speckle: single pixels of the other slope's plane (or unroofed) inside the two slopes, never two adjacent and never
    # beside a pixel of another plane (such a pixel would belong to the other slope's facet)
    rng = np.random.default_rng(5)
    pad = np.pad(r.roof, 1, constant_values=-9)
    inner = np.logical_and.reduce([pad[1 + dy:pad.shape[0] - 1 + dy, 1 + dx:pad.shape[1] - 1 + dx] == r.roof
                                   for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0))])
    ys, xs = np.nonzero((b.map == house) & ((r.roof == pw) | (r.roof == pe)) & inner)
    pick = (ys % 3 == 0) & (xs % 3 == 0) & (rng.random(len(ys)) < 0.5)
    noisy = r.roof.copy()
    noisy[ys[pick], xs[pick]] = np.where(rng.random(pick.sum()) < 0.2, 0, np.where(noisy[ys[pick], xs[pick]] == pw, pe, pw))
    assert pick.sum() >= 20
    rn = dataclasses.replace(r, roof=noisy)
    base_z, flat = api._solid_defaults(b, None, None)
    c = dict(bmap=b.map, roof=noisy, n_buildings=b.n_buildings, normal=r.normal, center=r.center, z_min=r.z_min, z_max=r.z_max,
             bin=r.bin, base_z=base_z, flat=flat, params=cases.params(min_pixels=16, merge_flat=True))
    g = ctx.generalise_roofs(b.map, rn, b, **c["params"])
    want = cases.run_ref(c)
    assert gr.same(g, want) is None, gr.same(g, want)
    # the facets of the house are the two slopes: the speckle is gone, and so are the specks of a wall plane along the
    # eaves that the vote itself leaves there (the result is the one of the unspeckled image)
    g0 = ctx.generalise_roofs(b.map, r, b, **c["params"])
    on_house = b.map == house
    assert np.array_equal(g.roof[on_house], g0.roof[on_house]) and g.converged == 1 and g.pixels_roofed == (noisy[ys[pick], xs[pick]] == 0).sum()
    assert g.building_facets_out[house] == 2 and sorted(set(g.roof[on_house].tolist())) == sorted([pw, pe])
    assert g.building_facets_in[house] > 2 + pick.sum() // 2
    print("gabled scene: house facets", g.building_facets_in[house], "->", g.building_facets_out[house], "rounds", g.rounds,
          "sum |dtop|", g.building_sum_abs_dtop[house], "max |dtop|", g.building_max_abs_dtop[house])
    # downstream, with and without the stage
    counts = {}
    for tag, roofs in (("noisy", rn), ("generalised", g.roofs)):
        s = ctx.solids(b.map, roofs, b)
        rf = ctx.roof_structure(b.map, roofs, s)
        p, t, o, plain = ctx.building_model(rf, s, tolerance_mm=0)
        wp, _, wc = uref.clean(rf.facet, s.top, rf.n_facets, 0, 1)
        wantp = pref.poly_solids(wp, wc, tref.triangulate(wp, wc), rf.facet_building, s.n_buildings, s.bin, s.base_z)
        assert pref.same(p, wantp) is None, (tag, pref.same(p, wantp))
        check_promises(p, s.bin)
        assert tag == "noisy" or p.n_open_buildings == 0
        counts[tag] = (rf.n_facets, o.n_svertices, p.n_vertices)
    print("gabled scene: (facets, clean vertices, model vertices)", counts)
    assert counts["generalised"][0] < counts["noisy"][0] and counts["generalised"][1] < counts["noisy"][1]
    assert counts["generalised"][2] < counts["noisy"][2]
    # solid_model(generalise=...) on the unspeckled cloud: the default changes nothing, the dict returns the generalised Roofs
    _, _, r2, s2 = ctx.solid_model(xyz, plane_idx, planes, refit=True, generalise=dict(min_pixels=16, merge_flat=True))
    assert np.array_equal(r2.roof, g0.roof) and np.array_equal(s2.top, ctx.solids(b.map, g0.roofs, b).top)
    assert np.array_equal(s0.top, ctx.solids(b.map, r, b).top)
