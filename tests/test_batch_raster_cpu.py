"""Host side of the raster / footprint batches (bs_grid_dims_batch and the Python helpers), without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = {"bs_tile_boxes_dev", "bs_grid_dims_batch", "bs_grid_picture_batch_dev", "bs_grid_picture_batch",
       "bs_footprints_batch_dev", "bs_footprints_batch"}


def _dims_batch(ext, bin_=100):
    ext = np.ascontiguousarray(ext, dtype=np.int32)
    nt = len(ext)
    w, h, po = np.zeros(nt, np.int32), np.zeros(nt, np.int32), np.zeros(nt + 1, np.int64)
    rc = _lib.load().bs_grid_dims_batch(ext.ctypes.data, nt, bin_, w.ctypes.data, h.ctypes.data, po.ctypes.data)
    return rc, w, h, po


def test_batch_exports_are_declared_and_loaded():
    txt = open(os.path.join(os.path.dirname(HERE), "include", "bs_api.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(bs_[a-z_]+)\s*\(", txt))
    assert NEW <= declared and NEW <= set(_lib.EXPORTS)
    L = _lib.load()
    for s in NEW:
        assert hasattr(L, s), s
    # no context: every context call refuses, no GPU needed
    assert L.bs_grid_picture_batch(None, None, None, 1, None, 100, 1000, None, None) == -1
    assert L.bs_footprints_batch(None, None, None, None, 1, 10, 5, 2, None, None, None, None) == -1
    assert L.bs_tile_boxes_dev(None, None, None, 1, None) == -1


@pytest.mark.parametrize("bin_", [1, 37, 100, 1000])
def test_dims_batch_equals_solo_dims(bin_):
    rng = np.random.default_rng(bin_)
    ext = rng.integers(0, 60_000, (50, 3)).astype(np.int32)
    ext[3] = 0
    ext[7, :2] = [bin_ - 1, bin_]
    rc, w, h, po = _dims_batch(ext, bin_)
    assert rc == 0
    for t in range(len(ext)):
        assert (w[t], h[t]) == api.grid_dims(ext[t], bin_)
    assert po[0] == 0 and np.array_equal(po[1:], np.cumsum(w.astype(np.int64) * h))
    pw, ph, ppo = api.grid_dims_batch(ext, bin_)
    assert np.array_equal(pw, w) and np.array_equal(ph, h) and np.array_equal(ppo, po)


def test_dims_batch_large_offsets_are_int64():
    ext = np.full((3, 3), 3_000_000, np.int32)  # 30 002 x 30 002 pixels per tile: the sum passes 2^31
    rc, w, h, po = _dims_batch(ext, 100)
    assert rc == 0 and po[-1] == 3 * 30002 * 30002 > 2 ** 31


@pytest.mark.parametrize("t", [0, 3, 9])
@pytest.mark.parametrize("bad", ["x", "y"])
def test_dims_batch_bad_extent_in_tile_t(t, bad):
    ext = np.full((10, 3), 1000, np.int32)
    ext[t, 0 if bad == "x" else 1] = -1
    assert _dims_batch(ext)[0] == -1
    with pytest.raises(ValueError):
        api.grid_dims_batch(ext)


@pytest.mark.parametrize("bin_", [0, -5])
def test_dims_batch_bad_bin(bin_):
    assert _dims_batch(np.full((4, 3), 1000, np.int32), bin_)[0] == -1
    with pytest.raises(ValueError):
        api.grid_dims_batch(np.full((4, 3), 1000), bin_)


def test_dims_batch_null_and_empty():
    L = _lib.load()
    w = np.zeros(1, np.int32)
    po = np.zeros(2, np.int64)
    ext = np.zeros((1, 3), np.int32)
    assert L.bs_grid_dims_batch(None, 1, 100, w.ctypes.data, w.ctypes.data, po.ctypes.data) == -1
    assert L.bs_grid_dims_batch(ext.ctypes.data, 0, 100, w.ctypes.data, w.ctypes.data, po.ctypes.data) == -1
    assert L.bs_grid_dims_batch(ext.ctypes.data, 1, 100, w.ctypes.data, w.ctypes.data, None) == -1


@pytest.mark.parametrize("ext,err", [([], ValueError), (np.zeros((0, 3)), ValueError), (np.zeros((2, 2)), ValueError),
                                     (np.zeros(3), ValueError), (np.full((2, 3), 1.5), TypeError),
                                     ([[0, 0, 0], [2 ** 31, 0, 0]], ValueError), ([[0, -1, 0]], ValueError)])
def test_python_dims_batch_validates(ext, err):
    with pytest.raises(err):
        api.grid_dims_batch(ext)


def test_python_batch_methods_validate_before_the_device():
    ctx = object.__new__(api.Context)  # no device: the checks come before any library call
    img = np.zeros((4, 5, 3))
    for bad in ([], np.zeros((2, 4, 5, 3)), [img, np.zeros((4, 5))], [img, np.zeros((0, 5, 3))], [np.zeros((4, 5, 2))]):
        with pytest.raises(ValueError):
            ctx.footprints_batch(bad)
    with pytest.raises(ValueError):
        ctx.footprints_batch_dev(0, [3, 4], [3])
    with pytest.raises(ValueError):
        ctx.footprints_batch_dev(0, [], [])
    tiles = [np.zeros((3, 3), np.int32), np.ones((2, 3), np.int32)]
    with pytest.raises(ValueError):
        ctx.grid_picture_batch(tiles, extents=np.zeros((3, 3), np.int32))  # one extent per tile
    with pytest.raises(ValueError):
        ctx.grid_picture_batch([])
    with pytest.raises(ValueError):
        ctx.grid_picture_batch_dev(0, [0, 3, 5], np.zeros((1, 3), np.int32), 0)
    with pytest.raises(ValueError):
        ctx.tile_boxes_dev(0, [0])


def test_footprint_view_of_a_batch_writes_the_solo_bytes(tmp_path):
    """The header's promise: a per-tile view {offset + co[t], same xy} writes what the solo result writes."""
    rng = np.random.default_rng(1)
    lens = [4, 7, 5, 3, 6]
    xy = rng.integers(0, 40, (sum(lens), 2)).astype(np.int32)
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    co = [0, 2, 2, 5]  # three tiles: 2 contours, none, 3
    wh = [(41, 40), (9, 9), (50, 43)]
    L = _lib.load()
    for t in range(3):
        a, b = co[t], co[t + 1]
        view = _lib.Contours()
        view.n_contours, view.width, view.height = b - a, *wh[t]
        view.offset = C.cast(off.ctypes.data + 8 * a, C.POINTER(C.c_int64))
        view.xy = xy.ctypes.data_as(C.POINTER(C.c_int32))
        assert L.bs_contours_write_obj(C.byref(view), str(tmp_path / "view.obj").encode()) == 0
        solo = api.Footprints([xy[off[i]:off[i + 1]] for i in range(a, b)], np.zeros(b - a), np.zeros(b - a), *wh[t])
        api.write_footprints_obj(solo, tmp_path / "solo.obj")
        assert (tmp_path / "view.obj").read_bytes() == (tmp_path / "solo.obj").read_bytes()
