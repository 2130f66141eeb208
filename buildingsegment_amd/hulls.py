"""Oriented boxes: the convex hull and the minimum-area enclosing rectangle of every label of a label image
(bs_label_hulls, include/bs_api.h), through the C ABI like everything in api.py and with its shared helpers.  The functions
take the api.Context to run on:

    hulls.label_hulls(ctx, label, n_labels=None) -> LabelHulls
    hulls.label_hulls_dev(ctx, d_label, width, height, n_labels) -> LabelHulls (hull_xy None)
    hulls.label_hulls_emit_dev(ctx, d_hull_xy)
    hulls.building_boxes(ctx, bmap, n_buildings=None) -> LabelHulls
    hulls.write_boxes_obj(hulls, path, bin, origin=None)
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import BsError
from .api import _columns, _copy, _copy_arrays, _fill, _label_top, _origin, _ptr, _write_obj


@dataclass
class LabelHulls:
    """bs_label_hulls: the totals, the layout figures (info), the per-label arrays and the hull vertices hull_xy (None after
    label_hulls_dev) as include/bs_api.h names them.  Label l has the hull vertices hull_offset[l] .. hull_offset[l + 1].
    The float conveniences are computed from the integers and are NaN (corners: an error) for a label that is not
    BS_HULL_OK."""
    width: int
    image_height: int
    n_labels: int
    n_hull_vertices: int
    n_ok: int
    n_empty: int
    n_too_large: int
    status: np.ndarray
    box: np.ndarray
    pixels2: np.ndarray
    n_hull: np.ndarray
    hull_offset: np.ndarray
    hull_area2: np.ndarray
    best_edge: np.ndarray
    dir: np.ndarray
    len2: np.ndarray
    a_min: np.ndarray
    a_max: np.ndarray
    c_max: np.ndarray
    area_num: np.ndarray
    info: dict = field(default_factory=dict)
    hull_xy: np.ndarray | None = field(default=None, repr=False)

    def _over(self, num, den):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(self.status == 0, np.asarray(num, np.float64) / np.asarray(den, np.float64), np.nan)

    @property
    def angle_deg(self):
        """the direction of the rectangle's sides in [0, 90) degrees from the X axis"""
        a = np.degrees(np.arctan2(self.dir[:, 1].astype(np.float64), self.dir[:, 0].astype(np.float64))) % 90.0
        return np.where(self.status == 0, np.where(a >= 90.0, 0.0, a), np.nan)

    def _sides(self):
        root = np.sqrt(self.len2.astype(np.float64))
        return self._over(self.a_max - self.a_min, root), self._over(self.c_max, root)

    @property
    def long_side(self):
        return np.fmax(*self._sides())

    @property
    def short_side(self):
        return np.fmin(*self._sides())

    @property
    def rectangularity(self):
        """pixel area / rectangle area"""
        return self._over(self.pixels2.astype(np.float64) * self.len2, 2.0 * self.area_num.astype(np.float64))

    @property
    def convexity(self):
        """pixel area / hull area"""
        return self._over(self.pixels2, self.hull_area2)

    def corners(self, l, bin=1, origin=None):
        """the four corners [4][2] (int64) of label l's rectangle through bs_hull_box_corners: lattice units times bin, plus
        origin [2 or 3]"""
        if self.hull_xy is None:
            raise ValueError("LabelHulls.corners: the hull vertices are on the device")
        st, keep = _label_hulls_struct(self)
        org = None if origin is None else np.ascontiguousarray(origin, dtype=np.int32).reshape(-1)
        if org is not None and len(org) not in (2, 3):
            raise ValueError("LabelHulls.corners: origin must be [2] or [3]")
        out = np.zeros((4, 2), np.int64)
        rc = _lib.load().bs_hull_box_corners(C.byref(st), int(l), int(bin), _ptr(org), out.ctypes.data)
        if rc != 0:
            raise BsError(rc, f"LabelHulls.corners: label {l} has no rectangle, or bin < 1")
        return out


# (name, dtype, columns) of the per-label arrays of bs_label_hulls (hull_offset has one entry more)
_HULL_ARRAYS = tuple((k, np.dtype(t), c) for k, t, c in _lib.HULL_ARRAYS if k != "hull_offset")


def _take_label_hulls(L, out, vertices) -> LabelHulls:
    """Copy a bs_label_hulls into numpy arrays and release it."""
    try:
        nl, nv = out.n_labels, out.n_hull_vertices
        arrs = _copy_arrays(out, _HULL_ARRAYS, nl)
        arrs["hull_offset"] = _copy(out.hull_offset, (nl + 1,), np.int64)
        info = {k: getattr(out, k) for k in _lib.HULL_LAYOUT + _lib.HULL_MS}
        return LabelHulls(out.width, out.height, nl, nv, out.n_ok, out.n_empty, out.n_too_large, info=info,
                          hull_xy=_copy(out.hull_xy, (nv, 2), np.int32) if vertices else None, **arrs)
    finally:
        L.bs_label_hulls_free(C.byref(out))


def _label_hulls_struct(h):
    """a bs_label_hulls over the arrays of a LabelHulls (or anything with its names), and the arrays to keep alive"""
    st, keep = _lib.LabelHulls(), []
    st.n_labels, st.n_hull_vertices = int(h.n_labels), int(h.n_hull_vertices)
    st.n_ok, st.n_empty, st.n_too_large = int(h.n_ok), int(h.n_empty), int(h.n_too_large)
    _fill(st, h, "LabelHulls", _columns(_HULL_ARRAYS, st.n_labels) + [("hull_offset", np.int64, st.n_labels + 1),
          ("hull_xy", np.int32, 2 * st.n_hull_vertices)], keep)
    return st, keep


def label_hulls(ctx, label, n_labels=None):
    """The convex hull and the minimum-area enclosing rectangle of every label of a label image ([height][width],
    negative = outside) on the api.Context ctx.  n_labels defaults to label.max() + 1.  Returns LabelHulls."""
    label, _, h, w, nl = _label_top("label_hulls", label, None, n_labels)
    out = _lib.LabelHulls()
    ctx._check(ctx._L.bs_label_hulls(ctx._h, label.ctypes.data, w, h, nl, C.byref(out)))
    return _take_label_hulls(ctx._L, out, True)


def label_hulls_dev(ctx, d_label, width, height, n_labels):
    """Device-resident count (bs_label_hulls_count_dev): d_label is a device pointer (int).  Returns LabelHulls with
    hull_xy None and the size n_hull_vertices of the buffer label_hulls_emit_dev fills."""
    out = _lib.LabelHulls()
    ctx._check(ctx._L.bs_label_hulls_count_dev(ctx._h, d_label or None, width, height, int(n_labels), C.byref(out)))
    return _take_label_hulls(ctx._L, out, False)


def label_hulls_emit_dev(ctx, d_hull_xy):
    """The hull vertices of the last label_hulls_dev on this context into a device buffer (int) of exactly its size:
    d_hull_xy [n_hull_vertices][2]."""
    ctx._check(ctx._L.bs_label_hulls_emit_dev(ctx._h, d_hull_xy or None))


def building_boxes(ctx, bmap, n_buildings=None):
    """label_hulls() of a building map (Context.building_map(): -1 outside, else the building): the direction every
    building faces and its oriented rectangle."""
    return label_hulls(ctx, bmap, n_labels=n_buildings)


def write_boxes_obj(hulls, path, bin, origin=None):
    """The hull and the rectangle of every BS_HULL_OK label of a LabelHulls as an OBJ of closed polylines in millimetres
    through the library's writer (bs_hull_boxes_write_obj; the format is written down in include/bs_api.h).  origin: the
    shift that was subtracted from the cloud."""
    if hulls.hull_xy is None:
        raise ValueError("write_boxes_obj: the hull vertices are on the device")
    st, keep = _label_hulls_struct(hulls)
    _write_obj("bs_hull_boxes_write_obj", path, "the hull arrays do not fit each other", C.byref(st), int(bin), _origin(origin))
