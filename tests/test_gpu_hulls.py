"""Oriented boxes on the device (bs_label_hulls, bs_label_hulls_count_dev / _emit_dev; include/bs_api.h) against the
definition in Python integers (tests/hull_ref/brute.py); the layout figures against the numpy restatement of the device pass
(tests/hull_ref/hull_ref.py).  Everything is an exact integer: every comparison is ==.  The sparse cases (compared products
around and above 2^64, coordinates at the bound, round counts around the batch) are built for what tests/test_hulls_cpu.py
asserts of them; DESIGN.md "Oriented boxes under test" has the list and what a changed line of the kernels fails.

The guarded-scratch test runs under test_gpu_scratch_guard's own `guarded` contexts, so that the slots of bs_ctx::hl count in
that module's coverage assertion (which runs after this file in a run of the whole suite)."""
import ctypes as C

import numpy as np
import pytest

from buildingsegment_amd import _lib, api, hulls

from test_hulls_cpu import FUZZ, MAGNITUDE, NAMED, ROUNDS, SPARSE, SPARSE_FUZZ, brute, cases, sparse_pair  # noqa: E402

pytestmark = pytest.mark.gpu
LAYOUT = ("n_candidates", "rounds", "max_live")
PATTERN = -0x5A5A5A5B  # no lattice coordinate of the cases


def check(ctx, c, want=None, ref=None, layout=True):
    """the host-memory entry point against the definition, its layout figures against the restatement"""
    want = cases.run_brute(c) if want is None else want
    ref = cases.run_ref(c) if ref is None and layout else ref
    got = hulls.label_hulls(ctx, c[0], n_labels=c[1])
    assert brute.same(got, want) is None, brute.same(got, want)
    assert (got.n_labels, got.width, got.image_height) == (c[1],) + c[0].shape[::-1]
    if layout:
        assert {k: got.info[k] for k in LAYOUT} == ref.info
    brute.identities(got)
    return got


def check_sparse(ctx, name):
    """a sparse case: the image for the device, the two references from its pixel list (tests/test_hulls_cpu.py asserts what
    the case was built for)"""
    return check(ctx, cases.dense(SPARSE[name]), *sparse_pair(name))


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case(gpu_ctx, name):
    check(gpu_ctx, NAMED[name])


@pytest.mark.parametrize("name", sorted(FUZZ))
def test_fuzz(gpu_ctx, name):
    check(gpu_ctx, FUZZ[name])


@pytest.mark.parametrize("name", sorted(MAGNITUDE))
def test_magnitude_case(gpu_ctx, name):
    """the compared products on both sides of 2^64 (high words zero, different, equal, the tie), the coordinates at the bound
    of either axis, a small label beside a huge one"""
    check_sparse(gpu_ctx, name)


@pytest.mark.parametrize("name", sorted(ROUNDS))
def test_round_case(gpu_ctx, name):
    """5, 8, 9 and 13 rounds against the batch of 4 between two reads of the live count; labels of 1, 5 and 9 together"""
    got = check_sparse(gpu_ctx, name)
    assert got.info["rounds"] == (9 if name == "rounds_1_5_9" else int(name.split("_")[1]))


@pytest.mark.parametrize("name", sorted(SPARSE_FUZZ))
def test_sparse_fuzz(gpu_ctx, name):
    check_sparse(gpu_ctx, name)


def test_full_bound(gpu_ctx):
    """a box of 16383 x 16383 in an image of 16384 x 16384: both coordinates at the bound, compared products up to 2^84.8.
    Against the definition from the pixel list alone."""
    check(gpu_ctx, cases.dense(cases.full_bound()), sparse_pair("full_bound")[0], layout=False)


def test_figures_of_the_shapes(gpu_ctx):
    """what the definition says about the shapes, asked of the device: the discs' hull sizes and tied edges, the parabolas on
    both sides of the 64 lanes of the box pass, the square's four tied edges, the rotated rectangles' directions"""
    for r, (n_hull, edge) in cases.DISCS.items():
        got = hulls.label_hulls(gpu_ctx, *cases.disc(r))
        assert (got.n_hull[0], got.best_edge[0]) == (n_hull, edge)
    for j in cases.PARABOLAS:
        assert hulls.label_hulls(gpu_ctx, *cases.parabola(j)).n_hull[0] == j + 5
    sq = hulls.label_hulls(gpu_ctx, *NAMED["square"])
    assert (sq.n_hull[0], sq.best_edge[0], sq.area_num[0]) == (4, 0, 36 * sq.len2[0])
    for d, a, b, n in cases.ROTATED:
        got = hulls.label_hulls(gpu_ctx, *cases.rotated(d, a, b, n))
        dx, dy = (int(v) for v in got.dir[0])
        assert dx * d[1] - dy * d[0] == 0 or dx * d[0] + dy * d[1] == 0, (d, dx, dy)
        assert 0 <= got.angle_deg[0] < 90 and got.long_side[0] >= got.short_side[0] > 0
        assert 0 < got.rectangularity[0] <= got.convexity[0] <= 1


def test_moving_a_label(gpu_ctx):
    for name in ("L", "disc_12", "rotated_7_3_33x20"):
        a, b = hulls.label_hulls(gpu_ctx, *NAMED[name]), hulls.label_hulls(gpu_ctx, *cases.moved(NAMED[name], 5, 3))
        for k in brute.PER_LABEL + brute.TOTALS:
            if k != "box":
                assert np.array_equal(getattr(a, k), getattr(b, k)), (name, k)
        assert np.array_equal(a.box + [5, 3, 5, 3], b.box) and np.array_equal(a.hull_xy + [5, 3], b.hull_xy)


def test_serpentine_many_candidates_small_hull(gpu_ctx):
    """257 x 257, one ring of more than 2^16 half-edges, a hull of 4"""
    c = cases.serpentine()
    got = check(gpu_ctx, c)
    assert got.n_hull.tolist() == [4] and got.info["n_candidates"] > 256


def test_large_image_with_blobs(gpu_ctx):
    """1025 x 1027: more than one sweep of the grid-stride passes underneath, more than 1 000 labels"""
    c = cases.blobs()
    got = check(gpu_ctx, c)
    assert got.n_ok > 1000 and got.info["n_candidates"] > 4 * got.n_ok - 1


def test_the_bound(gpu_ctx):
    got = check(gpu_ctx, cases.bound())
    assert got.status.tolist() == [brute.TOO_LARGE, brute.OK] and got.n_hull.tolist() == [0, 4]
    for k in ("hull_area2", "best_edge", "len2", "a_min", "a_max", "c_max", "area_num"):
        assert getattr(got, k)[0] == 0, k
    assert got.box[0].tolist() == [0, 0, 16385, 1] and np.isnan(got.angle_deg[0]) and not np.isnan(got.angle_deg[1])
    only = np.zeros((2, 16385), np.int32)  # no label within the bound: no candidate at all
    got = check(gpu_ctx, (only, 1))
    assert got.status.tolist() == [brute.TOO_LARGE] and got.info["n_candidates"] == 0 and got.n_hull_vertices == 0


# ---- device pointers --------------------------------------------------------------------------------------------------
def test_emit_twice_and_before_any_count(gpu_ctx):
    import torch
    fresh = api.Context(0)
    try:
        with pytest.raises(api.BsError) as e:
            hulls.label_hulls_emit_dev(fresh, torch.zeros(8, dtype=torch.int32, device="cuda").data_ptr())
        assert e.value.status == -1
    finally:
        fresh.close()
    lab, nl = NAMED["three_far_pieces"]
    want = cases.run_brute((lab, nl))
    d_label = torch.from_numpy(lab).cuda()
    got = hulls.label_hulls_dev(gpu_ctx, d_label.data_ptr(), lab.shape[1], lab.shape[0], nl)
    assert got.hull_xy is None and got.n_hull_vertices == want.n_hull_vertices
    for _ in range(2):
        d_xy = torch.full((got.n_hull_vertices + 1, 2), PATTERN, dtype=torch.int32, device="cuda")
        hulls.label_hulls_emit_dev(gpu_ctx, d_xy.data_ptr())
        torch.cuda.synchronize()
        xy = d_xy.cpu().numpy()
        assert np.array_equal(xy[:-1], want.hull_xy) and (xy[-1] == PATTERN).all()
    got.hull_xy = want.hull_xy
    assert brute.same(got, want) is None
    # the same round with products above 2^64 and a 4096 x 4096 image
    lab, nl = cases.dense(SPARSE["ladder_4096"])
    want = sparse_pair("ladder_4096")[0]
    d_label = torch.from_numpy(lab).cuda()
    got = hulls.label_hulls_dev(gpu_ctx, d_label.data_ptr(), lab.shape[1], lab.shape[0], nl)
    assert got.hull_xy is None and got.n_hull_vertices == want.n_hull_vertices == 8
    d_xy = torch.full((got.n_hull_vertices + 1, 2), PATTERN, dtype=torch.int32, device="cuda")
    hulls.label_hulls_emit_dev(gpu_ctx, d_xy.data_ptr())
    torch.cuda.synchronize()
    xy = d_xy.cpu().numpy()
    assert np.array_equal(xy[:-1], want.hull_xy) and (xy[-1] == PATTERN).all()
    got.hull_xy = want.hull_xy
    assert brute.same(got, want) is None


def test_errors_leave_out_untouched_and_the_context_usable(gpu_ctx):
    import torch
    L = _lib.load()
    lab, nl = NAMED["L"]
    d_label = torch.from_numpy(lab).cuda()
    h, w = lab.shape
    out = _lib.LabelHulls()
    out.n_labels = 12345
    for args, status in (((None, w, h, nl, C.byref(out)), -1), ((d_label.data_ptr(), w, h, nl, None), -1),
                         ((d_label.data_ptr(), 0, h, nl, C.byref(out)), -1), ((d_label.data_ptr(), w, 0, nl, C.byref(out)), -1),
                         ((d_label.data_ptr(), w, h, -1, C.byref(out)), -1), ((d_label.data_ptr(), w, h, 0, C.byref(out)), -2)):
        assert L.bs_label_hulls_count_dev(gpu_ctx._h, *args) == status, args
        assert out.n_labels == 12345 and not out.status
        with pytest.raises(api.BsError):  # a failed count leaves nothing to emit
            hulls.label_hulls_emit_dev(gpu_ctx, d_label.data_ptr())
    assert L.bs_label_hulls_count_dev(None, d_label.data_ptr(), w, h, nl, C.byref(out)) == -1
    assert L.bs_label_hulls(gpu_ctx._h, None, w, h, nl, C.byref(out)) == -1
    with pytest.raises(api.BsError) as e:
        hulls.label_hulls(gpu_ctx, lab, n_labels=0)
    assert e.value.status == -2
    check(gpu_ctx, NAMED["L"])


# ---- guarded scratch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_far_pieces", "parabola_64", "high_word"])
def test_guarded_scratch(gpu_ctx, name):
    """canary and poison on: the same result, no damaged guard, and every slot of bs_ctx::hl allocated"""
    from test_gpu_scratch_guard import POISON, guarded
    run = (lambda ctx: check(ctx, NAMED[name])) if name in NAMED else (lambda ctx: check_sparse(ctx, name))
    plain = run(gpu_ctx)
    for poison in POISON:
        with guarded(poison) as ctx:
            got = run(ctx)
            assert brute.same(got, plain, LAYOUT) is None
            assert ctx.selftest_scratch_check()["n_damaged"] == 0
            slots = {s["name"] for s in ctx.selftest_scratch_list()}
            assert {f"hl[{i}]" for i in range(25)} <= slots, sorted(slots)


# ---- pipeline -------------------------------------------------------------------------------------------------------------
def test_building_boxes_of_the_three_box_scene(gpu_ctx):
    from test_ground_cpu import cases as ground_cases
    xyz = ground_cases.scene(0)
    fp, b = gpu_ctx.buildings(xyz, bin=100)
    assert b.n_buildings == 3
    got = hulls.building_boxes(gpu_ctx, b.map, n_buildings=b.n_buildings)
    want = cases.run_brute((b.map, b.n_buildings))
    assert brute.same(got, want) is None and got.n_ok == 3
    brute.identities(got)
    assert (got.rectangularity > 0).all() and (got.convexity <= 1).all()
