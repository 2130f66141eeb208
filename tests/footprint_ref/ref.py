"""ctypes binding of contour_ref.c, the sequential CPU restatement of extracted_contour that the footprint tests
compare the device against.  The shared object is compiled next to the source on first use (git-ignored)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "contour_ref.c")
SO = os.path.join(HERE, "libcontour_ref.so")


class RefContours(C.Structure):
    _fields_ = [("n_contours", C.c_int32), ("offset", C.POINTER(C.c_int64)), ("xy", C.POINTER(C.c_int32)),
                ("area", C.POINTER(C.c_double)), ("perimeter", C.POINTER(C.c_double))]


_L = None


def lib():
    global _L
    if _L is not None:
        return _L
    if not os.path.exists(SO) or os.path.getmtime(SO) < os.path.getmtime(SRC):
        tmp = SO + f".{os.getpid()}.tmp"
        subprocess.check_call(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-ffp-contract=off", SRC, "-o", tmp, "-lm"])
        os.replace(tmp, SO)
    L = C.CDLL(SO)
    vp, rp = C.c_void_p, C.POINTER(RefContours)
    L.ref_mask.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp]
    L.ref_ellipse.argtypes = [C.c_int, vp]
    L.ref_close.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.ref_find_contours.argtypes = [vp, C.c_int, C.c_int, rp]
    L.ref_contours_free.argtypes = [rp]
    L.ref_contours_free.restype = None
    L.ref_write_obj.argtypes = [rp, C.c_int, C.c_int, C.c_char_p]
    L.ref_footprints.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, rp]
    _L = L
    return L


def ellipse(s):
    k = np.zeros((s, s), np.uint8)
    lib().ref_ellipse(s, k.ctypes.data)
    return k


def mask(image, threshold=10):
    img = np.ascontiguousarray(image, dtype=np.float64)
    h, w, _ = img.shape
    out = np.empty((h, w), np.uint8)
    lib().ref_mask(img.ctypes.data, w, h, threshold, out.ctypes.data)
    return out


def close(m, kernel_size=5, iterations=2):
    m = np.ascontiguousarray(m != 0, dtype=np.uint8).copy()
    h, w = m.shape
    lib().ref_close(m.ctypes.data, w, h, kernel_size, iterations)
    return m


class Result:
    """contours (list of (n, 2) int32 [x, y]), area, perimeter, width, height; write_obj(path)."""

    def __init__(self, rc: RefContours, w, h):
        n = rc.n_contours
        off = np.ctypeslib.as_array(rc.offset, (n + 1,)).copy()
        tot = int(off[-1])
        xy = np.ctypeslib.as_array(rc.xy, (2 * tot,)).reshape(tot, 2).copy() if tot else np.zeros((0, 2), np.int32)
        self.contours = [xy[off[i]:off[i + 1]] for i in range(n)]
        self.area = np.ctypeslib.as_array(rc.area, (n,)).copy() if n else np.zeros(0)
        self.perimeter = np.ctypeslib.as_array(rc.perimeter, (n,)).copy() if n else np.zeros(0)
        self.width, self.height = w, h
        self._off, self._xy = off, xy

    def write_obj(self, path):
        rc = RefContours()
        rc.n_contours = len(self.contours)
        rc.offset = self._off.ctypes.data_as(C.POINTER(C.c_int64))
        xy = np.ascontiguousarray(self._xy, dtype=np.int32)
        rc.xy = xy.ctypes.data_as(C.POINTER(C.c_int32))
        assert lib().ref_write_obj(C.byref(rc), self.width, self.height, str(path).encode()) == 0


def find_contours(m):
    m = np.ascontiguousarray(m != 0, dtype=np.uint8)
    h, w = m.shape
    rc = RefContours()
    assert lib().ref_find_contours(m.ctypes.data, w, h, C.byref(rc)) == 0
    try:
        return Result(rc, w, h)
    finally:
        lib().ref_contours_free(C.byref(rc))


def footprints(image, threshold=10, kernel_size=5, iterations=2):
    """(Result, closed mask 0 / 1) of the whole stage on a [h][w][3] f64 raster."""
    img = np.ascontiguousarray(image, dtype=np.float64)
    h, w, _ = img.shape
    m = np.empty((h, w), np.uint8)
    rc = RefContours()
    assert lib().ref_footprints(img.ctypes.data, w, h, threshold, kernel_size, iterations, m.ctypes.data,
                                C.byref(rc)) == 0
    try:
        return Result(rc, w, h), m
    finally:
        lib().ref_contours_free(C.byref(rc))


def image_of_mask(m):
    """A channel-1 raster whose threshold-10 mask is m: 0 and 30 (the tests' way to feed any mask to the tracer)."""
    m = np.asarray(m) != 0
    img = np.zeros(m.shape + (3,), np.float64)
    img[..., 1] = np.where(m, 30.0, 0.0)
    return img
