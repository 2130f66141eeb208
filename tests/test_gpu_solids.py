"""Solids on the device (bs_solids, bs_solids_count_dev, bs_solids_emit_dev; include/bs_api.h) against the numpy
restatement tests/solid_ref.  The one division of the height function apart everything is an exact integer, and the
division is the same IEEE operation on both sides: every comparison is ==."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "solid_ref"))
import solid_ref as sr  # noqa: E402
from test_roofs_cpu import load_roof_scenes  # noqa: E402
from test_solids_cpu import check_obj, check_solid, load_solid_cases  # noqa: E402

cases = load_solid_cases()

pytestmark = pytest.mark.gpu
I32_MIN = sr.I32_MIN


def tables(c):
    """what Context.solids takes from a Roofs"""
    return SimpleNamespace(roof=c["roof"], normal=c["normal"], center=c["center"], z_min=c["z_min"], z_max=c["z_max"], bin=c["bin"])


def run(ctx, c):
    return ctx.solids(c["bmap"], tables(c), base_z=c["base_z"], flat=c["flat"])


def check(ctx, c):
    got, want = run(ctx, c), cases.run_ref(c)
    assert sr.same(got, want) is None, sr.same(got, want)
    return got


SHAPES = cases.named_shapes()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_named_shape(gpu_ctx, name):
    check(gpu_ctx, SHAPES[name])


@pytest.mark.parametrize("w,h", [(1, 63), (63, 1), (64, 65), (65, 64), (257, 1), (1, 257), (257, 63), (63, 257), (64, 64),
                                 (65, 257), (257, 65)])
def test_image_sizes(gpu_ctx, w, h):
    check(gpu_ctx, cases.blob_case(w, h, seed=w * 1000 + h, size=7))


def test_large_image_with_blobs(gpu_ctx):
    """1025 x 1027: more pixels and more corners than one sweep of the grid-stride passes (4096 workgroups of 256), and
    many tiles of the scans; properties (a) and (b) from the device's arrays"""
    c = cases.blob_case(1025, 1027, seed=5, size=40, nb=700)
    assert 1025 * 1027 > 4096 * 256
    got = check(gpu_ctx, c)
    assert got.n_wall_faces > 0 and got.n_pixels > 500000
    check_solid(got, c["n_buildings"], c["bin"], got.volume6)


@pytest.mark.parametrize("nb", [cases.FIG_CAP - 1, cases.FIG_CAP, cases.FIG_CAP + 1, 5 * cases.FIG_CAP - 3])
def test_buildings_around_the_figure_tables(gpu_ctx, nb):
    got = check(gpu_ctx, cases.grid_of_buildings(nb, seed=nb))
    assert got.n_buildings == nb and (got.pixels == 1).all()


def test_planes_the_clamps_decide_and_tops_below_base(gpu_ctx):
    nan = float("nan")
    normal = np.array([[0, 0, 1.0], [30.0, -20.0, 0.5], [0.1, nan, 1.0], [0.1, 0.1, 0.0], [0.1, 0.1, -1.0], [0.0, 0.0, 1.0],
                       [0.5, 0.5, 1.0]])
    center = np.array([[0, 0, 500], [80, 80, 500], [0, 0, 500], [0, 0, 500], [40, 40, 500], [0, 0, -300], [0, 0, 2 ** 30]],
                      np.int32)
    z_min = np.array([0, 100, 200, 300, 400, -1000, sr.I32_MAX], np.int32)
    z_max = np.array([1000, 900, 800, 700, 600, 1000, sr.I32_MIN], np.int32)
    rng = np.random.default_rng(3)
    bmap = np.where(rng.random((40, 50)) < 0.85, rng.integers(0, 2, (40, 50)), -1)
    c = cases.make(bmap, rng.integers(0, 8, (40, 50)), 2, normal, center, z_min, z_max, 10, 150, [100, 900])
    got = check(gpu_ctx, c)
    r = cases.regimes(c)
    assert {"nan_plane", "nz_not_positive", "clamp_min", "clamp_max", "below_base", "top_at_base"} <= r
    assert got.top_min.min() == 150  # base_z wins over plane 6 (-300) and flat[0] (100)


def test_no_planes_everything_is_flat(gpu_ctx):
    c = cases.blob_case(70, 40, seed=2)
    c = cases.make(c["bmap"], np.zeros((40, 70)), c["n_buildings"], np.zeros((0, 3)), np.zeros((0, 3)), [], [], 10, 100, c["flat"])
    got = check(gpu_ctx, c)
    inb = c["bmap"] >= 0
    assert (got.top[inb] == np.maximum(100, c["flat"][c["bmap"][inb]])[:, None]).all() and (got.top[~inb] == I32_MIN).all()


@pytest.mark.parametrize("seed", range(cases.N_FUZZ))
def test_fuzz(gpu_ctx, seed):
    check(gpu_ctx, cases.fuzz_case(seed))


# ---- device pointers --------------------------------------------------------------------------------------------------
def dev_run(ctx, c, with_top):
    import torch
    h, w = c["bmap"].shape
    d_map, d_roof = torch.from_numpy(c["bmap"]).cuda(), torch.from_numpy(c["roof"]).cuda()
    d_top = torch.full((h, w, 4), 7, dtype=torch.int32, device="cuda") if with_top else None
    torch.cuda.synchronize()  # (the context has a stream of its own)
    s = ctx.solids_dev(d_map.data_ptr(), d_roof.data_ptr(), w, h, c["normal"], c["center"], c["z_min"], c["z_max"], c["bin"],
                       c["base_z"], c["flat"], d_top=d_top.data_ptr() if with_top else 0)
    assert s.vertex is None and s.face_index is None
    vertex = torch.full((max(s.n_vertices, 1), 4), -7, dtype=torch.int32, device="cuda")
    off = torch.full((s.n_faces + 1,), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((max(s.n_indices, 1),), -7, dtype=torch.int32, device="cuda")
    fb = torch.full((max(s.n_faces, 1),), -7, dtype=torch.int32, device="cuda")
    kind = torch.full((max(s.n_faces, 1),), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.solids_emit_dev(vertex.data_ptr(), off.data_ptr(), idx.data_ptr(), fb.data_ptr(), kind.data_ptr())
    torch.cuda.synchronize()
    s.vertex, s.face_offset = vertex.cpu().numpy()[:s.n_vertices], off.cpu().numpy()
    s.face_index, s.face_building = idx.cpu().numpy()[:s.n_indices], fb.cpu().numpy()[:s.n_faces]
    s.face_kind = kind.cpu().numpy()[:s.n_faces]
    s.top = d_top.cpu().numpy() if with_top else None
    return s


@pytest.mark.parametrize("with_top", [False, True])
def test_device_pointers(gpu_ctx, with_top):
    c = cases.fuzz_case(3)
    got, want = dev_run(gpu_ctx, c, with_top), cases.run_ref(c)
    names = (("top",) if with_top else ()) + sr.MESH + sr.FIGURES + sr.TOTALS
    assert sr.same(got, want, names) is None, sr.same(got, want, names)
    # the emit may be repeated, and another count replaces the offsets it reads
    c2 = cases.fuzz_case(5)
    assert sr.same(dev_run(gpu_ctx, c2, False), cases.run_ref(c2), sr.MESH + sr.FIGURES + sr.TOTALS) is None


# ---- errors -----------------------------------------------------------------------------------------------------------
def count_raw(ctx, c, dev, **kw):
    """bs_solids_count_dev on the device pointers dev = (d_map, d_roof, d_top), single arguments replaced by kw: returns
    (status, the bs_solids)"""
    h, w = c["bmap"].shape
    d_map, d_roof, d_top = dev
    a = dict(d_map=d_map, d_roof=d_roof, width=w, height=h, n_buildings=c["n_buildings"], n_planes=len(c["z_min"]),
             normal=c["normal"].ctypes.data, center=c["center"].ctypes.data, z_min=c["z_min"].ctypes.data,
             z_max=c["z_max"].ctypes.data, bin=c["bin"], base_z=c["base_z"], flat=c["flat"].ctypes.data, d_top=d_top)
    a.update(kw)
    out = _lib.Solids()
    rc = ctx._L.bs_solids_count_dev(ctx._h, a["d_map"] or None, a["d_roof"] or None, a["width"], a["height"], a["n_buildings"],
                                    a["n_planes"], a["normal"] or None, a["center"] or None, a["z_min"] or None,
                                    a["z_max"] or None, a["bin"], a["base_z"], a["flat"] or None, a["d_top"] or None,
                                    C.byref(out))
    return rc, out


def test_error_paths(gpu_ctx):
    import torch
    ctx = gpu_ctx
    c = cases.fuzz_case(1)
    h, w = c["bmap"].shape
    want = cases.run_ref(c)
    d_map, d_roof = torch.from_numpy(c["bmap"]).cuda(), torch.from_numpy(c["roof"]).cuda()
    d_top = torch.full((h, w, 4), 7, dtype=torch.int32, device="cuda")
    bufs = [torch.full((n,), 5, dtype=torch.int32, device="cuda") for n in (4 * want.n_vertices, want.n_faces + 1,
                                                                            want.n_indices, want.n_faces)]
    kind = torch.full((want.n_faces,), 5, dtype=torch.uint8, device="cuda")
    emit = lambda: ctx._L.bs_solids_emit_dev(ctx._h, *[b.data_ptr() for b in bufs], kind.data_ptr())  # noqa: E731
    torch.cuda.synchronize()  # (the context has a stream of its own)

    def untouched():
        torch.cuda.synchronize()
        return bool((d_top == 7).all()) and all(bool((b == 5).all()) for b in bufs + [kind])

    with api.Context(0) as fresh:  # emit before any count
        assert fresh._L.bs_solids_emit_dev(fresh._h, *[b.data_ptr() for b in bufs], kind.data_ptr()) == -1
        assert b"count" in fresh._L.bs_last_error(fresh._h)
    # BS_ERR_INVALID
    for kw in (dict(d_map=0), dict(d_roof=0), dict(width=0), dict(height=0), dict(height=-3), dict(bin=0), dict(n_buildings=-1),
               dict(n_planes=-1), dict(flat=0), dict(normal=0), dict(center=0), dict(z_min=0), dict(z_max=0)):
        rc, out = count_raw(ctx, c, (d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr()), **kw)
        assert rc == -1, kw
        assert out.n_faces == 0 and not out.pixels
    assert untouched()
    assert ctx._L.bs_solids_count_dev(ctx._h, d_map.data_ptr(), d_roof.data_ptr(), w, h, c["n_buildings"], 0, None, None, None,
                                      None, c["bin"], 0, c["flat"].ctypes.data, None, None) == -1  # out == NULL
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
        rc, out = count_raw(ctx, c, (dm.data_ptr(), dr.data_ptr(), d_top.data_ptr()))
        assert rc == -2 and out.n_faces == 0 and not out.pixels, what
        assert emit() == -1, what  # emit after a failed count
        assert untouched(), what
        with pytest.raises(api.BsError) as e:  # the host-memory twin reports the same
            ctx.solids(m, SimpleNamespace(**{**vars(tables(c)), "roof": r}), base_z=c["base_z"], flat=c["flat"])
        assert e.value.status == -2
    # a successful count makes the last failure forgotten: the context is as usable as before
    rc, out = count_raw(ctx, c, (d_map.data_ptr(), d_roof.data_ptr(), d_top.data_ptr()))
    assert rc == 0 and (out.n_vertices, out.n_faces, out.n_indices) == (want.n_vertices, want.n_faces, want.n_indices)
    ctx._L.bs_solids_free(C.byref(out))
    assert ctx._L.bs_solids_emit_dev(ctx._h, bufs[0].data_ptr(), 0, bufs[2].data_ptr(), bufs[3].data_ptr(), kind.data_ptr()) == -1
    assert emit() == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_top.cpu().numpy(), want.top) and np.array_equal(bufs[2].cpu().numpy(), want.face_index)
    assert np.array_equal(bufs[0].cpu().numpy().reshape(-1, 4), want.vertex) and np.array_equal(kind.cpu().numpy(), want.face_kind)
    check(ctx, cases.fuzz_case(9))


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_gabled_scene_end_to_end(gpu_ctx, tmp_path):
    sc = load_roof_scenes()
    xyz = sc.gabled()
    _, _, plane_idx, planes = gpu_ctx.segment(xyz, api.default_params(k=15))
    fp, b, r, s = gpu_ctx.solid_model(xyz, plane_idx, planes, refit=True)
    assert r.fit is not None and b.n_buildings == 3 == s.n_buildings and s.bin == 100
    base = int(b.ground_th)
    q = np.abs(b.z_sum) // np.maximum(b.n_above, 1) * np.sign(b.z_sum)
    flat = np.where(b.n_above > 0, q, base)
    assert s.base_z == base
    want = sr.solids(b.map, r.roof, 3, r.normal, r.center, r.z_min, r.z_max, 100, base, flat)
    assert sr.same(s, want) is None, sr.same(s, want)
    c = dict(n_buildings=3, bin=100)
    check_solid(s, 3, 100, s.volume6)  # every building closed, volume6 == the determinant sum
    assert (s.pixels > 0).all() and np.array_equal(s.pixels, b.pixels)
    assert (s.pixels * (s.top_min.astype(np.int64) - base) * 6 <= s.volume6).all()
    assert (s.volume6 <= s.pixels * (s.top_max.astype(np.int64) - base) * 6).all()
    row, cols = sc.gable_pixels()
    ridge = s.top[row, cols].max()
    assert sc.EAVES - 200 <= s.top[row, cols].min() and sc.RIDGE - 200 <= ridge <= sc.RIDGE + 200
    data = check_obj(s, c, str(tmp_path / "solids.obj"))
    assert data.startswith(b"# solids: 3 buildings, ")
