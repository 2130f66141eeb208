"""Buildings (include/bs_api.h, "buildings") without a GPU: the C-ABI surface, the host-only LoD1 OBJ writer against
its Python restatement, and the numpy / scipy restatement of the building map (tests/building_ref) against the
sequential contour restatement (tests/footprint_ref): building c is contour c."""
import ctypes as C
import glob
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
sys.path.insert(0, os.path.join(HERE, "building_ref"))
import building_ref as bref  # noqa: E402
import ref  # noqa: E402
import scenes  # noqa: E402

from buildingsegment_amd import api, synth  # noqa: E402
from test_gpu_footprints import SHAPES  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "raster_*.npz")))
NEW = ["bs_building_map_dev", "bs_building_map", "bs_buildings_free", "bs_assign_buildings_dev", "bs_assign_buildings",
       "bs_plane_buildings_dev", "bs_plane_buildings", "bs_buildings_write_obj"]


def test_new_symbols_are_declared_loaded_and_exported():
    from buildingsegment_amd import _lib, build
    import test_abi
    build.build()
    L = _lib.load()
    declared = test_abi._declared()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.bs_api_version() == 5
    st = _lib.Buildings()
    L.bs_buildings_free(C.byref(st))  # a zeroed struct is accepted
    assert st.n_buildings == 0


def _fp(contours, area, perimeter, w=100, h=80):
    cs = [np.asarray(c, np.int32).reshape(-1, 2) for c in contours]
    return api.Footprints(cs, np.asarray(area, float), np.asarray(perimeter, float), w, h)


def _bld(n_above, z_sum):
    n = len(n_above)
    z = np.zeros
    return api.Buildings(n, 100, 80, z((n, 2), np.int32), z((n, 4), np.int32), z(n, np.int64), z(n, np.int64),
                         np.asarray(n_above, np.int64) + 3, np.asarray(n_above, np.int64), z(n, np.int32), z(n, np.int32),
                         np.asarray(z_sum, np.int64))


CONTOURS = [
    [[3, 2], [3, 5], [6, 5], [6, 2]],  # kept
    [[10, 10], [10, 40], [40, 40], [40, 10]],  # area too small (see AREA)
    [[7, 7]],  # one point, kept: two degenerate quads, no roof
    [[50, 1], [70, 1]],  # two points, kept: no roof
    [[20, 60], [20, 70], [30, 75], [40, 70], [40, 60]],  # perimeter too small
    [[1, 1], [1, 9], [9, 9]],  # no above-ground point
    [[60, 60], [60, 70], [70, 70]],  # kept, negative height sum: the quotient truncates towards zero
    [[80, 10], [80, 20], [90, 20], [90, 10]],  # area == min_area: not kept (strict)
]
AREA = [900.0, 100.0, 501.0, 777.5, 5000.0, 800.0, 600.0, 500.0]
PERIM = [120.0, 300.0, 100.5, 101.0, 100.0, 400.0, 200.0, 150.0]
N_ABOVE = [7, 9, 1, 4, 5, 0, 3, 2]
Z_SUM = [70001, 90000, 12345, 39999, 50, 0, -10, 40]


@pytest.mark.parametrize("origin", [None, (0, 0, 0), (431200, 5620000, 87000), (-4321, -99, -20)],
                         ids=["null", "zero", "positive", "negative"])
@pytest.mark.parametrize("ground_th,bin_", [(3000.0, 100), (0.0, 37), (-2500.0, 1)])
def test_write_obj_bytes_equal_the_restatement(tmp_path, origin, ground_th, bin_):
    fp, b = _fp(CONTOURS, AREA, PERIM), _bld(N_ABOVE, Z_SUM)
    api.write_buildings_obj(fp, b, tmp_path / "b.obj", bin=bin_, origin=origin, ground_th=ground_th)
    got = (tmp_path / "b.obj").read_bytes()
    want = bref.obj_text(fp.contours, AREA, PERIM, N_ABOVE, Z_SUM, bin_, origin, ground_th)
    assert got == want
    assert got.startswith(b"# buildings: 4 of 8\n")
    assert got.count(b"\nv ") == 2 * (4 + 1 + 2 + 3) and got.count(b"\nf ") == (4 + 1 + 2 + 3) + 2


def test_write_obj_filters_and_errors(tmp_path):
    fp, b = _fp(CONTOURS, AREA, PERIM), _bld(N_ABOVE, Z_SUM)
    api.write_buildings_obj(fp, b, tmp_path / "all.obj", ground_th=1.0, min_area=0.0, min_perimeter=0.0)
    assert (tmp_path / "all.obj").read_bytes() == bref.obj_text(fp.contours, AREA, PERIM, N_ABOVE, Z_SUM, 100, None, 1.0,
                                                                 0.0, 0.0)
    assert (tmp_path / "all.obj").read_bytes().startswith(b"# buildings: 7 of 8\n")
    api.write_buildings_obj(fp, b, tmp_path / "none.obj", ground_th=1.0, min_area=1e9)
    assert (tmp_path / "none.obj").read_bytes() == b"# buildings: 0 of 8\n"
    api.write_buildings_obj(_fp([], [], []), _bld([], []), tmp_path / "empty.obj", ground_th=1.0)
    assert (tmp_path / "empty.obj").read_bytes() == b"# buildings: 0 of 0\n"
    with pytest.raises(api.BsError) as e:  # the contours and the buildings are not of the same mask
        api.write_buildings_obj(fp, _bld(N_ABOVE[:3], Z_SUM[:3]), tmp_path / "x.obj", ground_th=1.0)
    assert e.value.status == -1
    with pytest.raises(api.BsError):
        api.write_buildings_obj(fp, b, tmp_path / "x.obj", bin=0, ground_th=1.0)
    with pytest.raises(api.BsError):
        api.write_buildings_obj(fp, b, tmp_path / "no_such_dir" / "x.obj", ground_th=1.0)


def _agree(mask):
    """count, start pixels and map[contour point] == c against the contour restatement"""
    r = ref.find_contours(mask)
    b = bref.building_map(mask)
    assert b.n_buildings == len(r.contours)
    assert [tuple(c[0]) for c in r.contours] == [tuple(s) for s in b.start_xy.tolist()]
    for c, pts in enumerate(r.contours):
        assert (b.map[pts[:, 1], pts[:, 0]] == c).all()
    m = np.asarray(mask) != 0
    assert (b.map[m] >= 0).all()  # the foreground always belongs to a building
    assert b.pixels.sum() == (b.map >= 0).sum() and b.fg_pixels.sum() == m.sum()
    assert (b.bbox[:, 0] <= b.start_xy[:, 0]).all() and (b.bbox[:, 1] == b.start_xy[:, 1]).all()
    return b


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("k", [0, 2])
def test_restatement_agrees_with_the_contours_on_shapes(name, k):
    m = SHAPES[name] if k == 0 else ref.close(SHAPES[name], 5, k)
    b = _agree(m)
    if name == "blobs3" and k == 0:
        assert b.n_buildings == 14330
    if name == "nested" and k == 0:  # the blob in the innermost hole belongs to the outer ring's building
        assert b.n_buildings == 1 and b.map[30, 30] == 0 and b.pixels[0] == 62 * 62 and b.fg_pixels[0] < 62 * 62


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_restatement_agrees_with_the_contours_on_golden_rasters(path):
    _, mask = ref.footprints(np.load(path)["image"])
    _agree(mask)


@pytest.mark.parametrize("scene", ["urban", "boxes", "composed"])
def test_restatement_on_scenes_and_above_ground_is_assigned(oracle, scene):
    xyz = {"urban": lambda: synth.shift_to_origin(synth.urban(150_000, seed=11)),
           "boxes": lambda: synth.shift_to_origin(synth.boxes(n_boxes=6)),
           "composed": scenes.composed}[scene]()
    img, th = oracle.grid_picture(xyz)
    _, mask = ref.footprints(img)
    b = _agree(mask)
    a = bref.assign(xyz, b.map, b.n_buildings, 100, th)
    assert a.above.any() and (a.building_idx[a.above] >= 0).all()
    assert a.n_points.sum() == (a.building_idx >= 0).sum()
    if scene == "composed":  # the kinds the device test of this scene needs
        assert b.n_buildings >= 8 and (a.building_idx < 0).any()
        px, py = xyz[:, 0] // 100, xyz[:, 1] // 100
        assert bref.enclosed_pixels(mask, b.map)[py, px].any()


def test_votes_restatement_by_hand():
    plane = np.array([1, 1, 1, 2, 2, 2, 2, 3, -1, 4, 4, 9], np.int32)
    bidx = np.array([0, 1, 1, 2, 2, 0, 0, -1, 1, 1, -1, 0], np.int32)
    pb, vin, tot, out = bref.votes(plane, bidx, 5, 3)
    assert pb.tolist() == [1, 0, -1, 1, -1]  # plane 2: a tie, the lower building wins; plane 3 lies outside
    assert vin.tolist() == [2, 2, 0, 1, 0] and tot.tolist() == [3, 4, 1, 2, 0] and out.tolist() == [0, 0, 1, 1, 0]
