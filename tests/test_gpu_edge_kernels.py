"""The O(N) device kernels either side of the hot path, each at its own boundaries and against the plain numpy restatement of
tests/edge_ref/edge_ref.py: ingest_kernel, minmax_kernel / shift_kernel, tile_bbox_kernel / tile_shift_kernel / tile_of,
color_scatter_kernel, owner_fetch_kernel / labels_from_owner_kernel, remap_rows_kernel / remap_rows_table_kernel and
cc_hook_kernel / cc_compress_kernel.  The cases, and the boundary each one sits on, are in tests/edge_ref/cases.py;
tests/test_edge_kernels_cpu.py has asserted their premises and that every boundary has a case on each side.  Every comparison
is ==.  Each size is the smallest that crosses its boundary; the largest inputs are the remap's (2^22 entries: 16 MiB of rows,
16 MiB of output, a 12 MiB table)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tools"))

import fuzz_edges as F  # noqa: E402
from test_gpu_ingest import parse_binary  # noqa: E402

cases, ref = F.cases, F.ref
EDGE = np.load(os.path.join(HERE, "golden", "ply_edge_cases.npz"))
INVALID, RANGE = -1, -2
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def gold(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def eq(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64))


# ---- ingest ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 3])
@pytest.mark.parametrize("name", [f[0] for f in cases.PLY_EDGE_FILES])
def test_ingest_of_the_fixture_files_at_any_alignment(gpu_ctx, name, lead):
    """what the reference's reader made of the two files, with the body at an aligned pointer and 1 and 3 bytes behind one (an
    upload of a whole file hands the library a pointer just past the header)"""
    buf = EDGE[name + "/in"].tobytes()
    n, stride, pos, kind, end = parse_binary(buf)
    want = EDGE[name + "/xyz"]
    off, is64 = (pos["x"], pos["y"], pos["z"]), kind["x"] == "float64"
    got, mn = F.dev_ingest(gpu_ctx, buf[end:end + n * stride], n, stride, off, is64, 1000.0, False, lead)
    assert eq(got, want) and not mn.any()  # (no shift: the files span more than the 2^31 - 1 the shift's contract allows)


@pytest.mark.parametrize("n", cases.INGEST_N)
def test_ingest_of_every_layout(gpu_ctx, n):
    """strides 12 .. 40, three property orders, both widths, four scales, with and without the shift"""
    rng = np.random.default_rng(n)
    runs = 0
    for stride, order, is64, off in cases.ingest_layouts():
        for scale in cases.INGEST_SCALES:
            rec = cases.ingest_records(rng, n, stride, off, is64, scale)
            for shift in (False, True):
                want, wmn = F.want_ingest(rec, n, stride, off, is64, scale, shift)
                got, mn = F.dev_ingest(gpu_ctx, rec, n, stride, off, is64, scale, shift, lead=runs % 4)
                assert eq(got, want) and eq(mn, wmn), (stride, order, is64, scale, shift)
                runs += 1
    assert runs == 22 * 4 * 2


def _one_value_records(dt, n, at, value):
    """n records of three scalars of type dt (small whole numbers) with `value` at (record, axis) `at`"""
    v = (np.arange(3 * n, dtype=np.float64).reshape(n, 3) % 1000) - 500
    v = v.astype(dt)
    v[at] = value
    w = int(dt[2])
    return v.tobytes(), 3 * w, (0, w, 2 * w)


def test_ingest_ends_of_the_range(gpu_ctx):
    n = cases.INGEST_REJECT_N
    for value, dt, want_int in cases.INGEST_ENDS:
        for at in cases.INGEST_REJECT_AT:
            rec, stride, off = _one_value_records(dt, n, at, value)
            want, bad = ref.ingest(rec, n, stride, off, dt == "<f8", 1.0)
            assert not bad and want[at] == want_int
            got, mn = F.dev_ingest(gpu_ctx, rec, n, stride, off, dt == "<f8", 1.0, False)
            assert eq(got, want) and not mn.any(), (value, dt, at)


def _raw_ingest(ctx, rec, n, stride, off, is64, scale, shift, mn):
    """bs_ingest_dev with the caller's own min_out: (status, xyz)"""
    import torch
    body = F.to_dev(np.frombuffer(rec, np.uint8))
    d_xyz = torch.full((n, 3), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = ctx._L.bs_ingest_dev(ctx._h, body.data_ptr(), n, stride, off[0], off[1], off[2], 1 if is64 else 0, float(scale),
                              1 if shift else 0, d_xyz.data_ptr(), mn.ctypes.data)
    return rc, d_xyz.cpu().numpy()


@pytest.mark.parametrize("dt", ["<f8", "<f4"])
def test_ingest_rejects_what_does_not_fit(gpu_ctx, dt):
    """2^31, -2^31 - 1 (float32: the next one below -2^31), NaN and the infinities: BS_ERR_RANGE wherever they stand, min_out
    as it was, and the next good call on the same context correct"""
    n = cases.INGEST_REJECT_N
    good, stride, off = _one_value_records(dt, n, (0, 0), 7.0)
    want_good, wmn = F.want_ingest(good, n, stride, off, dt == "<f8", 1.0, True)
    for value in cases.INGEST_REJECTED[dt]:
        for at in cases.INGEST_REJECT_AT:
            rec, stride, off = _one_value_records(dt, n, at, value)
            assert ref.ingest(rec, n, stride, off, dt == "<f8", 1.0)[1]
            for shift in (True, False):
                mn = np.array([11, -22, 33], np.int32)
                rc, _ = _raw_ingest(gpu_ctx, rec, n, stride, off, dt == "<f8", 1.0, shift, mn)
                assert rc == RANGE and mn.tolist() == [11, -22, 33], (value, at, shift)
            mn = np.array([11, -22, 33], np.int32)
            rc, got = _raw_ingest(gpu_ctx, good, n, stride, off, dt == "<f8", 1.0, True, mn)
            assert rc == 0 and eq(got, want_good) and eq(mn, wmn), (value, at)


@pytest.mark.parametrize("dt", ["<f8", "<f4"])
def test_ingest_ignores_other_properties(gpu_ctx, dt):
    """the same values in a fourth scalar property of the record are none of the reader's business"""
    n, w = cases.INGEST_REJECT_N, int(dt[2])
    for value in cases.INGEST_REJECTED[dt]:
        v = ((np.arange(4 * n, dtype=np.float64).reshape(n, 4) % 1000) - 500).astype(dt)
        v[:, 1] = value  # x, other, y, z
        rec, off = v.tobytes(), (0, 2 * w, 3 * w)
        want, bad = ref.ingest(rec, n, 4 * w, off, dt == "<f8", 1.0)
        got, mn = F.dev_ingest(gpu_ctx, rec, n, 4 * w, off, dt == "<f8", 1.0, False)
        assert not bad and eq(got, want)


# ---- shift -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cases.SHIFT_N)
def test_shift_finds_the_minimum_wherever_it_sits(gpu_ctx, n):
    for place in cases.SHIFT_PLACES:
        xyz = cases.shift_cloud(n, place)
        want, wmn = ref.shift(xyz)
        got, mn = F.dev_shift(gpu_ctx, xyz)
        assert eq(mn, wmn) and eq(got, want), (n, place, cases.shift_min_indices(n, place))


def test_shift_of_further_clouds(gpu_ctx):
    for name, xyz in cases.shift_further_clouds():
        want, wmn = ref.shift(xyz)
        got, mn = F.dev_shift(gpu_ctx, xyz)
        assert eq(mn, wmn) and eq(got, want), name


def _segment_dev(ctx, d_xyz, n, k, bufs=None):
    import torch
    from buildingsegment_amd import api
    d_pl, d_ng, d_nr = bufs or (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, k), dtype=torch.int32, device="cuda"),
                                torch.empty((n, 3), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    ctx.segment_dev(d_xyz.data_ptr(), n, d_pl.data_ptr(), api.default_params(k=k), d_ng.data_ptr(), d_nr.data_ptr())
    planes = ctx.planes_fetch()
    return (d_pl, d_ng, d_nr), (d_pl.cpu().numpy(), d_ng.cpu().numpy(), d_nr.cpu().numpy().view(np.int64), planes)


def test_segment_again_after_a_shift_in_place(gpu_ctx):
    """segment, shift the same buffer in place, segment again with the same pointers and n: what a fresh context makes of the
    shifted cloud (a cell order cached for the pointer must not outlive the shift)"""
    from buildingsegment_amd import api
    g = gold("plane_cube_12k")
    raw = g["xyz"].astype(np.int64) + np.array([905_003, -257, 77])
    n, k = len(raw), g["neigh"].shape[1]
    d_xyz = F.to_dev(raw.astype(np.int32))
    bufs, first = _segment_dev(gpu_ctx, d_xyz, n, k)
    mn = gpu_ctx.shift_to_origin_dev(d_xyz.data_ptr(), n)
    shifted, wmn = ref.shift(raw)
    assert eq(mn, wmn) and wmn.any() and eq(d_xyz.cpu().numpy(), shifted)
    _, again = _segment_dev(gpu_ctx, d_xyz, n, k, bufs)
    with api.Context(0) as fresh:
        _, want = _segment_dev(fresh, F.to_dev(shifted.astype(np.int32)), n, k)
    for a, b in zip(again[:3], want[:3]):
        assert np.array_equal(a, b)
    assert len(again[3]) == len(want[3]) > 0
    for p, q in zip(again[3], want[3]):
        assert p.id == q.id and np.array_equal(p.pointIdx, q.pointIdx) and np.array_equal(p.center, q.center)
        assert np.array_equal(p.normal.view(np.int64), q.normal.view(np.int64))
    # (so far from the origin the reference's int32 coordinate sums wrap, as in tests/golden/walls_6k_overflow: the first call
    # solved another problem, and the second result is none of its left-overs)
    assert [len(p.pointIdx) for p in first[3]] != [len(p.pointIdx) for p in again[3]]


# ---- tile boxes and the tile shift -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", sorted(cases.TILE_BATCHES))
def test_tile_boxes_and_tile_shift(gpu_ctx, batch):
    xyz, off = cases.tile_batch(batch)
    wbox = ref.tile_boxes(xyz, off)
    wsh, wmn = ref.shift_tiles(xyz, off)
    box, mn, sh, box2 = F.dev_tiles(gpu_ctx, xyz, off)
    assert eq(box, wbox) and eq(mn, wmn) and eq(sh, wsh)
    wbox2 = ref.tile_boxes(wsh, off)
    assert eq(box2, wbox2) and not wbox2[:, :3].any()


# ---- colours -----------------------------------------------------------------------------------------------------------------
def _colours(ctx, rgb, n):
    import torch
    d_col = torch.full((n, 3), 999, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    ctx.plane_colors_dev(rgb, n, d_col.data_ptr())
    return d_col.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("rg_mode", [0, 1, 2])
def test_colours_after_segment_and_after_region_grow(gpu_ctx, rg_mode):
    import torch
    from buildingsegment_amd import api
    largest = 0
    for name in cases.COLOUR_CLOUDS:
        g = gold(name)
        xyz, k = g["xyz"], g["neigh"].shape[1]
        n = len(xyz)
        p = api.default_params(k=k, rg_mode=rg_mode)
        d_xyz = F.to_dev(xyz)
        d_pl, d_ng, d_nr = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty((n, k), dtype=torch.int32, device="cuda"),
                            torch.empty((n, 3), dtype=torch.float64, device="cuda"))
        torch.cuda.synchronize()
        gpu_ctx.segment_dev(d_xyz.data_ptr(), n, d_pl.data_ptr(), p, d_ng.data_ptr(), d_nr.data_ptr())
        planes = gpu_ctx.planes_fetch()
        rgb = cases.colour_table(len(planes), seed=rg_mode)
        want = ref.colours(n, [q.pointIdx for q in planes], rgb)
        assert np.array_equal(_colours(gpu_ctx, rgb, n), want)
        # the grower alone on the golden file's normals and rows: the planes the reference's own stage 3 wrote into the file
        d_nr, d_ng = F.to_dev(g["normals"]), F.to_dev(g["neigh"])
        gpu_ctx.region_grow_dev(d_xyz.data_ptr(), d_nr.data_ptr(), d_ng.data_ptr(), n, d_pl.data_ptr(), p)
        planes2 = gpu_ctx.planes_fetch()
        lists = [g["point_idx"][a:b] for a, b in zip(g["offset"][:-1], g["offset"][1:])]
        assert [q.pointIdx.tolist() for q in planes2] == [l.tolist() for l in lists] and eq(d_pl.cpu().numpy(), g["plane_idx"])
        rgb2 = cases.colour_table(len(lists), seed=rg_mode + 10)
        assert np.array_equal(_colours(gpu_ctx, rgb2, n), ref.colours(n, lists, rgb2))
        largest = max([largest] + [len(q.pointIdx) for q in planes] + [len(l) for l in lists])
    assert largest > cases.COLOUR_BIG_PLANE  # the scatter's loop over a plane's list made a second trip


def test_colours_after_a_batch_cover_the_concatenation(gpu_ctx):
    import torch
    from buildingsegment_amd import api
    tiles = [gold(name)["xyz"] for name in ("grid_patch_p1", "plane_cube_12k", "facade_10k_k16")]
    off = np.concatenate([[0], np.cumsum([len(t) for t in tiles])]).astype(np.int64)
    n = int(off[-1])
    d_xyz = F.to_dev(np.concatenate(tiles))
    d_pl = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    gpu_ctx.segment_batch_dev(d_xyz.data_ptr(), off, d_pl.data_ptr(), api.default_params(k=15))
    per_tile = gpu_ctx.batch_planes_fetch()
    assert len(per_tile) == 3 and len(per_tile[1]) > 0 and sum(len(p) > 0 for p in per_tile) >= 2
    lists = [q.pointIdx.astype(np.int64) + off[t] for t, pl in enumerate(per_tile) for q in pl]
    assert max(len(l) for l in lists) > cases.COLOUR_BIG_PLANE
    rgb = cases.colour_table(len(lists), seed=3)
    want = ref.colours(n, lists, rgb)
    assert np.array_equal(_colours(gpu_ctx, rgb, n), want)
    for t in range(3):  # a tile with planes is coloured, over its own part of the concatenation
        assert want[off[t]:off[t + 1]].any() == (len(per_tile[t]) > 0)


def test_colours_without_planes_and_refused_calls(gpu_ctx):
    import torch
    from buildingsegment_amd import api
    g = gold("walls_6k")
    xyz, n = g["xyz"], len(g["xyz"])
    d_xyz = F.to_dev(xyz)
    d_pl = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # no plane commits: d_colors all zero over the pattern
    gpu_ctx.segment_dev(d_xyz.data_ptr(), n, d_pl.data_ptr(), api.default_params(k=15, th_point_count=1_000_000))
    assert gpu_ctx.planes_fetch() == []
    assert not _colours(gpu_ctx, np.zeros((0, 3), np.int32), n).any()
    with pytest.raises(api.BsError) as e:
        _colours(gpu_ctx, np.zeros((1, 3), np.int32), n)
    assert e.value.status == INVALID
    # refusals leave d_colors alone
    gpu_ctx.segment_dev(d_xyz.data_ptr(), n, d_pl.data_ptr(), api.default_params(k=15))
    npl = len(gpu_ctx.planes_fetch())
    assert npl > 0
    d_col = torch.full((n, 3), 999, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    for rgb, nn in ((cases.colour_table(npl), n - 1), (cases.colour_table(npl), n + 1), (cases.colour_table(npl + 1), n),
                    (np.zeros((0, 3), np.int32), n)):
        with pytest.raises(api.BsError) as e:
            gpu_ctx.plane_colors_dev(rgb, nn, d_col.data_ptr())
        assert e.value.status == INVALID and (d_col.cpu().numpy() == 999).all()
    gpu_ctx.plane_colors_dev(cases.colour_table(npl), n, d_col.data_ptr())
    assert (d_col.cpu().numpy() != 999).all()


# ---- owners, seeds, labels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_seeds", cases.LABEL_N_SEEDS)
def test_labels_from_owner_of_every_kind(gpu_ctx, n_seeds):
    own, seeds, kinds = cases.label_case(n_seeds)
    assert eq(F.dev_labels(gpu_ctx, own, seeds), ref.labels_from_owner(own, seeds))
    for n in cases.LABEL_SMALL_N:
        own, seeds, _ = cases.label_case(n_seeds, n=n, seed=n)
        assert len(own) == n and eq(F.dev_labels(gpu_ctx, own, seeds), ref.labels_from_owner(own, seeds))


def test_owners_seeds_and_labels_of_the_scene(gpu_ctx, oracle):
    """owner_fetch after bs_segment_dev as well as after bs_region_grow_dev, rg_mode 0 and 2, on a scene that has labelled points
    whose owner committed nothing, owners below the first committed seed and above the last; plane_seeds below its count"""
    import torch
    from buildingsegment_amd import api, synth
    xyz = synth.boxes()
    n = len(xyz)
    ng, nr = oracle.knn_normals(xyz, k=15)
    pi, pl, ow = oracle.region_grow(xyz, nr, ng, want_owner=True)
    seeds = pl["point_idx"][pl["offset"][:-1]].astype(np.int32)
    lab = ow >= 0
    assert (~np.isin(ow[lab], seeds)).any() and (ow[lab] < seeds.min()).any() and (ow[lab] > seeds.max()).any()
    assert eq(ref.labels_from_owner(ow, seeds), np.where(lab, pi, -1))
    d_xyz, d_nr, d_ng = F.to_dev(xyz), F.to_dev(nr), F.to_dev(ng)
    d_lab = torch.empty(n, dtype=torch.int32, device="cuda")
    for rg_mode in (0, 2):
        p = api.default_params(k=15, rg_mode=rg_mode)
        for call in ("segment", "region_grow"):
            d_own = torch.full((n,), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            if call == "segment":
                gpu_ctx.segment_dev(d_xyz.data_ptr(), n, d_lab.data_ptr(), p)
            else:
                gpu_ctx.region_grow_dev(d_xyz.data_ptr(), d_nr.data_ptr(), d_ng.data_ptr(), n, d_lab.data_ptr(), p)
            gpu_ctx.owner_fetch_dev(d_own.data_ptr())
            gpu_ctx.sync()
            assert eq(d_lab.cpu().numpy(), pi) and eq(d_own.cpu().numpy(), ow), (rg_mode, call)
            npl = gpu_ctx.plane_seeds_dev(0, 0)
            assert npl == len(seeds) >= 3
            d_seeds = torch.full((npl,), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert gpu_ctx.plane_seeds_dev(d_seeds.data_ptr(), npl - 2) == npl  # the full count, whatever the room
            gpu_ctx.sync()
            assert eq(d_seeds.cpu().numpy(), np.concatenate([seeds[:npl - 2], [-9, -9]]))
            assert gpu_ctx.plane_seeds_dev(d_seeds.data_ptr(), npl) == npl
            gpu_ctx.sync()
            assert eq(d_seeds.cpu().numpy(), seeds)
            d_lab2 = torch.full((n,), -9, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            gpu_ctx.labels_from_owner_dev(d_own.data_ptr(), n, d_seeds.data_ptr(), npl, d_lab2.data_ptr())
            gpu_ctx.sync()
            assert eq(d_lab2.cpu().numpy(), pi)


# ---- remap -------------------------------------------------------------------------------------------------------------------
def _remap_input():
    def make():
        flat, sg = cases.remap_input()
        want, miss = ref.remap(flat, sg)
        assert not miss
        return flat, sg, want
    return memo("remap", make)


@pytest.mark.parametrize("k", cases.REMAP_K)
def test_remap_by_table_and_by_binary_search(gpu_ctx, k):
    """either side of 2^22 entries, with BS_REMAP_BSEARCH and without: the two paths give the same rows, the restatement's, and
    report a missing index exactly when there is one -- negative, last + 1, far above, inside the span but absent.  (The cap
    of 2^20 workgroups, 2^28 entries, is not reachable at test size.)"""
    flat, sg, want = _remap_input()
    d_flat, d_sg = F.to_dev(flat), F.to_dev(sg)
    missing = cases.remap_missing(sg)
    for n_rows in cases.REMAP_ROWS[k]:
        total = n_rows * k
        d_rows = d_flat[:total]
        for bsearch in (False, True):
            out, miss = F.dev_remap(gpu_ctx, d_rows, n_rows, k, d_sg, len(sg), bsearch)
            assert miss == 0 and eq(out, want[:total]), (n_rows, bsearch)
        for j, (kind, value) in enumerate((kind, v) for kind, vals in missing.items() for v in vals):
            at = (0, total - 1, total // 2 + 1)[j % 3]
            d_rows[at] = value
            w = want[:total].copy()
            w[at] = 0
            outs = [F.dev_remap(gpu_ctx, d_rows, n_rows, k, d_sg, len(sg), b) for b in (False, True)]
            d_rows[at] = int(flat[at])
            assert outs[0][1] != 0 and outs[1][1] != 0, (n_rows, kind, value)
            assert np.array_equal(outs[0][0], outs[1][0]) and eq(outs[0][0], w), (n_rows, kind, value)


def test_remap_into_an_empty_cloud(gpu_ctx):
    rows = np.arange(12, dtype=np.int32).reshape(4, 3)
    out, miss = F.dev_remap(gpu_ctx, F.to_dev(rows), 4, 3, F.to_dev(np.zeros(1, np.int32)), 0, False)
    want, wmiss = ref.remap(rows, np.zeros(0, np.int32))
    assert wmiss and miss != 0 and eq(out, want.reshape(-1))


# ---- hooking -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cases.HOOK_K)
def test_hook_of_one_rank(gpu_ctx, k):
    n = cases.HOOK_N_TOTAL
    for permuted in (False, True):
        gidx, rows = cases.hook_case(k, permuted)
        want = ref.components(n, gidx, rows)
        parent, hooks = F.dev_components(gpu_ctx, n, k, gidx, rows)
        assert hooks[-1] == 0 and len(hooks) >= 2
        assert eq(parent, want) and (parent <= np.arange(n)).all()
        assert sum(hooks) == n - int((want == np.arange(n)).sum())  # a forest of n nodes


@pytest.mark.parametrize("graph", cases.HOOK_GRAPHS)
@pytest.mark.parametrize("ranks", cases.HOOK_RANKS)
def test_hook_and_minimum_rounds_of_several_ranks(gpu_ctx, graph, ranks):
    """the protocol of include/bs_api.h stepped on one device: a parent array per rank, every round a hook per rank and then
    the elementwise minimum, until no rank hooks"""
    n, order, rows = cases.hook_graph(graph)
    deal = [(F.to_dev(g), F.to_dev(r)) for g, r in cases.hook_deal(order, rows, ranks)]

    def hook(d_rows, d_gidx, parent):
        d_p = F.to_dev(parent)
        h = F.dev_hook(gpu_ctx, n, 2, d_gidx, d_rows, d_p)
        parent[:] = d_p.cpu().numpy()
        return h
    parent, rounds, per_round = cases.hook_rounds(n, deal, hook, cap=n)
    assert per_round[-1] == 0 and 3 <= rounds < n  # (the cap is a condition of the loop, not a result)
    assert eq(parent, ref.components(n, order, rows)) and not parent.any()


# ---- fuzz --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", cases.FUZZ_ENTRIES)
def test_fuzz_of_every_entry_point(gpu_ctx, entry):
    runs, bad = F.run(gpu_ctx, [entry], cases.FUZZ_CASES)
    assert runs == 40 and bad == []
