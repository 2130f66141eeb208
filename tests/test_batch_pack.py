"""The host side of bs_segment_batch that runs without a GPU: packing a tile list into (concatenation, offsets) and
the per-tile origin shift of the host form."""
import numpy as np
import pytest

from buildingsegment_amd import api


def test_pack_tiles_layout():
    a = np.arange(12, dtype=np.int32).reshape(4, 3)
    b = np.full((2, 3), -7, dtype=np.int64)
    c = np.array([[1, 2, 3]], dtype=np.int16)
    xyz, off = api.pack_tiles([a, b, c])
    assert xyz.dtype == np.int32 and xyz.flags.c_contiguous and xyz.shape == (7, 3)
    assert off.dtype == np.int64 and off.tolist() == [0, 4, 6, 7]
    assert np.array_equal(xyz[0:4], a) and np.array_equal(xyz[4:6], b) and np.array_equal(xyz[6:7], c)
    xyz, off = api.pack_tiles((a,))  # any sequence, a batch of one included
    assert off.tolist() == [0, 4] and np.array_equal(xyz, a)


@pytest.mark.parametrize("bad, exc", [
    ([], ValueError),
    (np.zeros((4, 3), np.int32), ValueError),  # one array, not a list of tiles
    ([np.zeros((4, 2), np.int32)], ValueError),
    ([np.zeros(12, np.int32)], ValueError),
    ([np.zeros((4, 3), np.int32), np.zeros((0, 3), np.int32)], ValueError),
    ([np.zeros((4, 3), np.float64)], TypeError),
    ([np.array([[0, 0, 1 << 31]], np.int64)], ValueError),
    ([np.array([[0, 0, (1 << 32) - 1]], np.uint32)], ValueError),
])
def test_pack_tiles_rejects(bad, exc):
    with pytest.raises(exc):
        api.pack_tiles(bad)


def test_pack_tiles_names_the_tile():
    with pytest.raises(ValueError, match="tile 2"):
        api.pack_tiles([np.zeros((3, 3), np.int32)] * 2 + [np.zeros((3, 4), np.int32)])


def test_shift_tiles_to_origin_host():
    a = np.array([[5, 6, 7], [9, 3, 8]], np.int32)
    b = np.array([[-100, 2_000_000_000, 0]], np.int32)
    xyz, off = api.pack_tiles([a, b])
    out = api.shift_tiles_to_origin(xyz, off)
    assert out.dtype == np.int32
    assert out.tolist() == [[0, 3, 0], [4, 0, 1], [0, 0, 0]]
    with pytest.raises(ValueError):
        api.shift_tiles_to_origin(xyz, [0, 2, 2, 3])  # an empty tile
    with pytest.raises(ValueError):
        api.shift_tiles_to_origin(xyz, [0, 2])  # does not cover the points
