"""Python host mirror of the reference's call sites for the hot path.

Reference (paths relative to /root/reference/tmc3/):
    get_Normal_and_K_neighbor<15>(pointCloud, normal, neigh);   TMC3.cpp:215, my_function.h:48-85
    seg_plane h(pointCloud, normal, neigh, 15);                  TMC3.cpp:216, my_function.h:98-104
    vector<plane> planes = h.get_planes();                       TMC3.cpp:217, my_function.cpp:180-217
    h.set_plane_color(planes);                                   TMC3.cpp:218, my_function.cpp:260-275

Everything here goes through the C ABI (include/bs_api.h) into the HIP
library; nothing is computed in Python and there is no CPU fallback.
"""
from __future__ import annotations

import copy
import warnings
import ctypes as C
from contextlib import contextmanager, nullcontext
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import BsError, Contours, FootprintInfo, Params, Planes, Timings


def default_params(**kw) -> Params:
    p = Params()
    _lib.load().bs_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, v)
    return p


# ---- what every stage of the binding shares: copies out of the library's structs, pointers into it, the input checks -------
def _copy(ptr, shape, dtype):
    """An owned numpy copy of the library's array at ptr, or the empty array of that shape and dtype when an extent is 0."""
    if 0 in shape:
        return np.zeros(shape, dtype)
    a = np.ctypeslib.as_array(ptr, shape)
    if a.dtype != dtype:
        raise TypeError(f"a {a.dtype} array was to be copied as {np.dtype(dtype)}")
    return a.copy()


def _copy_arrays(out, table, n):
    """{name: _copy} of the arrays of the struct `out` that share the length n: table rows are (name, dtype, columns)"""
    return {name: _copy(getattr(out, name), (n, cols) if cols > 1 else (n,), dt) for name, dt, cols in table}


def _rows(names, dtype):
    """(name, dtype, 1) rows for _copy_arrays from the names of arrays of one dtype"""
    return tuple((k, np.dtype(dtype), 1) for k in names)


_PAD = np.zeros(4, np.int64)  # what an empty table points at: never a null pointer, never read


def _ptr(a):
    """the address of an optional array, None (a null pointer) for None"""
    return None if a is None else a.ctypes.data


def _ptr0(a):
    """the address of a table that may be empty"""
    return (a if a.size else _PAD).ctypes.data


def _fill(st, src, what, table, keep):
    """Point the array fields of the ctypes struct st at the arrays of src (a dataclass `what`, or anything with its names):
    table rows are (name, dtype, values).  The arrays the struct then reads go to `keep`, which must outlive it."""
    types = dict(st._fields_)
    for name, dt, n in table:
        a = np.ascontiguousarray(getattr(src, name), dtype=dt).reshape(-1)
        if len(a) != n:
            raise ValueError(f"{what}.{name} must hold {n} values")
        keep.append(a if len(a) else np.zeros(1, dt))
        setattr(st, name, keep[-1].ctypes.data_as(types[name]))
    return keep


def _columns(table, n):
    """(name, dtype, columns) rows over n entries as the (name, dtype, values) rows of _fill"""
    return [(name, dt, n * cols) for name, dt, cols in table]


def _points(who, xyz):
    xyz = np.ascontiguousarray(xyz, dtype=np.int32)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{who}: xyz must be [n][3]")
    return xyz


def _point_labels(who, name, labels, xyz):
    a = np.ascontiguousarray(labels, dtype=np.int32)
    if a.shape != (len(xyz),):
        raise ValueError(f"{who}: {name} must be [n]")
    return a


def _label_top(who, label, top, n_labels, need_top=False):
    """(label, top, h, w, n_labels) of a label image [height][width] and its optional top image [height][width][4]"""
    label = np.ascontiguousarray(label, dtype=np.int32)
    if label.ndim != 2 or label.size == 0:
        raise ValueError(f"{who}: label must be [height][width]")
    if top is None and need_top:
        raise ValueError(f"{who}: the stage needs a top image")
    if top is not None:
        top = np.ascontiguousarray(top, dtype=np.int32)
        if top.shape != label.shape + (4,):
            raise ValueError(f"{who}: top must be [height][width][4]")
    h, w = label.shape
    return label, top, h, w, max(int(label.max()) + 1, 0) if n_labels is None else int(n_labels)


def _origin(origin):
    org = None if origin is None else np.ascontiguousarray(origin, dtype=np.int32)
    if org is not None and org.shape != (3,):
        raise ValueError("origin must be [3]")
    return org


def _host_image(who, image, name, dev_form):
    if image is None:
        raise ValueError(f"{who}: the {name} image is on the device: use {dev_form}")
    return image


def _has_top(who, solids):
    if solids.top is None:
        raise ValueError(f"{who}: the Solids carry no top image (solids(top=True))")


def _facet_and_top(who, roof_facets, solids, dev_form):
    """what the pipeline conveniences need of roof_facets() and solids(): both images in host memory"""
    _host_image(who, roof_facets.facet, "facet", dev_form)
    _has_top(who, solids)


def _write_obj(fn, path, what, *args):
    """One OBJ writer of the library: fn(*args, path) with arrays passed by address (None: a null pointer), a status other
    than 0 as BsError."""
    rc = getattr(_lib.load(), fn)(*[_ptr(a) if a is None or isinstance(a, np.ndarray) else a for a in args],
                                  str(path).encode())
    if rc != 0:
        raise BsError(rc, f"cannot write {path}" + (f" (or {what})" if what else ""))


_FREES = {getattr(_lib, cls): f"bs_{name}_free" for cls, name in (
    ("Contours", "contours"), ("Buildings", "buildings"), ("Roofs", "roofs"), ("PlaneFits", "plane_fits"), ("Solids", "solids"),
    ("RoofGeneralise", "roof_generalise"), ("RoofFacets", "roof_facets"), ("Outlines", "outlines"),
    ("SimpleOutlines", "simple_outlines"), ("CleanOutlines", "clean_outlines"), ("OutlineTriangles", "outline_triangles"),
    ("PolySolids", "poly_solids"), ("ModelRaster", "model_raster"), ("PointResiduals", "point_residuals"),
    ("Terrain", "terrain"), ("Ground", "ground"))}


def _free(L, out):
    """release what the library allocated into the struct `out`"""
    getattr(L, _FREES[type(out)])(C.byref(out))


def _take_chain(L, *parts):
    """The tail of a form that hands several structs back: parts are (taker, struct, *arguments) in the order of the
    returned tuple.  Every struct is released exactly once: by its taker, or here if an earlier copy raised."""
    got = []
    try:
        for take, st, *args in parts:
            got.append(None)  # take() releases st itself, also when it raises
            got[-1] = take(L, st, *args)
    finally:
        for _, st, *_ in parts[len(got):]:
            _free(L, st)
    return tuple(got)


@dataclass
class Plane:
    """struct plane (my_function.h:25-30)."""
    id: int
    normal: np.ndarray
    center: np.ndarray
    pointIdx: np.ndarray = field(repr=False)


def _planes_to_list(P: Planes):
    n = P.n_planes
    if n == 0:
        return []
    off, ids = _copy(P.offset, (n + 1,), np.int64), _copy(P.id, (n,), np.int32)
    nrm, ctr = _copy(P.normal, (n, 3), np.float64), _copy(P.center, (n, 3), np.int32)
    pidx = _copy(P.point_idx, (int(off[n]),), np.int32)  # (copied once: every plane's pointIdx is its slice of this copy)
    return [Plane(int(ids[i]), nrm[i].copy(), ctr[i].copy(), pidx[off[i]:off[i + 1]]) for i in range(n)]


class Context:
    """bs_ctx wrapper: one HIP device, its stream and scratch buffers."""

    def __init__(self, device: int = 0):
        self._L = _lib.load()
        self._h = C.c_void_p()
        rc = self._L.bs_create(device, C.byref(self._h))
        if rc != 0:
            raise BsError(rc, "bs_create failed (is a gfx950 GPU visible?)")
        self.device = device
        self._screen_dev = None  # (pointer, width, height) while set_footprint_screen(device=True) holds

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.bs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise BsError(rc, self._L.bs_last_error(self._h).decode())

    def set_stream(self, stream_handle):
        self._check(self._L.bs_set_stream(self._h, C.c_void_p(stream_handle)))

    def timings(self) -> dict:
        t = Timings()
        self._check(self._L.bs_get_timings(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timings._fields_}

    # ---- host-buffer API ----------------------------------------------------
    def knn_normals(self, xyz, params: Params | None = None):
        p = params or default_params()
        xyz = _points("knn_normals", xyz)
        n = xyz.shape[0]
        neigh = np.empty((n, p.k), dtype=np.int32)
        normals = np.empty((n, 3), dtype=np.float64)
        self._check(self._L.bs_knn_normals(self._h, xyz.ctypes.data, n, C.byref(p), neigh.ctypes.data,
                                           normals.ctypes.data))
        return neigh, normals

    def knn_normals_halo(self, xyz_local, gidx, n_query, params: Params, cert_radius: float):
        """Slab form: the first n_query points are queries, the rest halo; returns
        (neigh with GLOBAL indices, normals, number of uncertified k-lists)."""
        xyz_local = np.ascontiguousarray(xyz_local, dtype=np.int32)
        gidx = np.ascontiguousarray(gidx, dtype=np.int32)
        n = xyz_local.shape[0]
        neigh = np.empty((n_query, params.k), dtype=np.int32)
        normals = np.empty((n_query, 3), dtype=np.float64)
        unc = C.c_int64(0)
        self._check(self._L.bs_knn_normals_halo(self._h, xyz_local.ctypes.data, gidx.ctypes.data, n, n_query,
                                                C.byref(params), neigh.ctypes.data, normals.ctypes.data,
                                                float(cert_radius), C.byref(unc)))
        return neigh, normals, unc.value

    def region_grow(self, xyz, normals, neigh, params: Params | None = None):
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        normals = np.ascontiguousarray(normals, dtype=np.float64)
        neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        p = params or default_params(k=neigh.shape[1])
        if neigh.shape[1] != p.k:
            raise ValueError("neigh width != params.k")
        n = xyz.shape[0]
        plane_idx = np.empty(n, dtype=np.int32)
        P = Planes()
        self._check(self._L.bs_region_grow(self._h, xyz.ctypes.data, normals.ctypes.data, neigh.ctypes.data,
                                           n, C.byref(p), plane_idx.ctypes.data, C.byref(P)))
        planes = _planes_to_list(P)
        self._L.bs_planes_free(C.byref(P))
        return plane_idx, planes

    def segment(self, xyz, params: Params | None = None):
        p = params or default_params()
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        n = xyz.shape[0]
        neigh = np.empty((n, p.k), dtype=np.int32)
        normals = np.empty((n, 3), dtype=np.float64)
        plane_idx = np.empty(n, dtype=np.int32)
        P = Planes()
        self._check(self._L.bs_segment(self._h, xyz.ctypes.data, n, C.byref(p), neigh.ctypes.data,
                                       normals.ctypes.data, plane_idx.ctypes.data, C.byref(P)))
        planes = _planes_to_list(P)
        self._L.bs_planes_free(C.byref(P))
        return neigh, normals, plane_idx, planes

    # ---- device-buffer API (raw device pointers, e.g. torch.Tensor.data_ptr()) ----
    def knn_normals_dev(self, d_xyz, n, d_neigh, d_normals, params, q_begin=0, q_end=None, d_gidx=0,
                        cert_radius=0.0):
        q_end = n if q_end is None else q_end
        unc = C.c_int64(0)
        self._check(self._L.bs_knn_normals_dev(self._h, d_xyz, d_gidx or None, n, q_begin, q_end,
                                               C.byref(params), d_neigh, d_normals or None, cert_radius,
                                               C.byref(unc)))
        return unc.value

    def region_grow_dev(self, d_xyz, d_normals, d_neigh, n, d_plane_idx, params):
        self._check(self._L.bs_region_grow_dev(self._h, d_xyz, d_normals, d_neigh, n, C.byref(params),
                                               d_plane_idx))

    def segment_dev(self, d_xyz, n, d_plane_idx, params, d_neigh=0, d_normals=0):
        self._check(self._L.bs_segment_dev(self._h, d_xyz, n, C.byref(params), d_neigh or None,
                                           d_normals or None, d_plane_idx))

    def shift_to_origin_dev(self, d_xyz, n):
        """buildingSeg ctor shift (TMC3.cpp:55-73) in place on the device; returns the minimum."""
        mn = np.zeros(3, dtype=np.int32)
        self._check(self._L.bs_shift_to_origin_dev(self._h, d_xyz, n, mn.ctypes.data))
        return mn

    def ingest_dev(self, d_records, n, stride, offsets, is_f64, d_xyz, scale=1000.0, shift_to_origin=True):
        """ply::read's position quantisation (ply.cpp:436-465) on a device-resident binary vertex body,
        optionally followed by the buildingSeg shift; returns the subtracted minimum."""
        mn = np.zeros(3, dtype=np.int32)
        self._check(self._L.bs_ingest_dev(self._h, d_records, n, stride, offsets[0], offsets[1], offsets[2],
                                          1 if is_f64 else 0, float(scale), 1 if shift_to_origin else 0, d_xyz,
                                          mn.ctypes.data))
        return mn

    def plane_colors_dev(self, plane_rgb, n, d_colors):
        rgb = np.ascontiguousarray(plane_rgb, dtype=np.int32).reshape(-1, 3)
        self._check(self._L.bs_plane_colors_dev(self._h, rgb.ctypes.data, len(rgb), n, d_colors))

    def grid_picture(self, xyz, extent=None, bin=100, bin_height=1000):
        """buildingSeg::compute_gird_picture (TMC3.cpp:123-174) of a cloud already shifted to
        its bounding-box origin.  Returns (image [height][width][3] f64, ground_th)."""
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        ext = np.ascontiguousarray(xyz.max(0) if extent is None else extent, dtype=np.int32)
        w, h = grid_dims(ext, bin)
        img = np.empty((h, w, 3), dtype=np.float64)
        th = C.c_double(0)
        self._check(self._L.bs_grid_picture(self._h, xyz.ctypes.data, len(xyz), ext.ctypes.data, bin, bin_height,
                                            img.ctypes.data, C.byref(th)))
        return img, th.value

    def grid_picture_dev(self, d_xyz, n, extent, d_image, bin=100, bin_height=1000):
        """Device-resident variant: d_xyz / d_image are device pointers (ints)."""
        ext = np.ascontiguousarray(extent, dtype=np.int32)
        th = C.c_double(0)
        self._check(self._L.bs_grid_picture_dev(self._h, d_xyz, n, ext.ctypes.data, bin, bin_height, d_image, C.byref(th)))
        return th.value

    def footprints(self, image, threshold=10, kernel_size=5, iterations=2, return_mask=False):
        """extracted_contour (my_function.cpp:8-57) on a [height][width][3] f64 raster of grid_picture: quantise
        channel 1 like save_image, threshold, close with the ellipse, findContours(RETR_EXTERNAL,
        CHAIN_APPROX_SIMPLE).  Returns a Footprints (contours: list of (n_i, 2) int32 [x, y] arrays, area,
        perimeter, info) and, with return_mask, the closed [height][width] uint8 mask (0 / 255) as well."""
        img = np.ascontiguousarray(image, dtype=np.float64)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("footprints: image must be [height][width][3]")
        h, w, _ = img.shape
        mask = np.empty((h, w), dtype=np.uint8) if return_mask else None
        out, inf = Contours(), FootprintInfo()
        self._check(self._L.bs_footprints(self._h, img.ctypes.data, w, h, threshold, kernel_size, iterations,
                                          _ptr(mask), C.byref(out), C.byref(inf)))
        fp = _take_contours(self._L, out, inf)
        return (fp, mask) if return_mask else fp

    def footprints_dev(self, d_image, width, height, threshold=10, kernel_size=5, iterations=2, d_mask=0):
        """Device-resident variant: d_image ([height][width][3] f64) and d_mask ([height][width] uint8, optional)
        are device pointers (ints); the contours come back in host memory."""
        out, inf = Contours(), FootprintInfo()
        self._check(self._L.bs_footprints_dev(self._h, d_image or None, width, height, threshold, kernel_size,
                                              iterations, d_mask or None, C.byref(out), C.byref(inf)))
        return _take_contours(self._L, out, inf)

    def selftest_center_div(self, c, n):
        """Device evaluation of (int32)((uint64)(int64)c / n) through csrc/bs_centerdiv.h."""
        c = np.ascontiguousarray(c, dtype=np.int32)
        n = np.ascontiguousarray(n, dtype=np.uint32)
        out = np.empty_like(c)
        self._check(self._L.bs_selftest_center_div(self._h, c.ctypes.data, n.ctypes.data, out.ctypes.data, len(c)))
        return out

    def selftest_forge_next(self, mode):
        """The next region grow corrupts one finished plane (1: duplicated entry, 2: normal off by an ulp);
        timings()['validation_rejects'] must then be >= 1 and the result still exact."""
        self._check(self._L.bs_selftest_forge_next(self._h, int(mode)))

    def set_audit(self, on=True):
        """Replay every plane attempt against the final owners after each region grow (see bs_set_audit);
        timings()['audit_mismatches'] must be 0."""
        self._check(self._L.bs_set_audit(self._h, 1 if on else 0))

    def selftest_grow_limits(self, max_waves=0, pool_cap=0, max_pending=0, pstore_cap=0, retry_max_list=-1,
                             retry_big_round=-1, full_refresh=False):
        """Lower the speculative grower's capacities for the following grows on this context (see
        bs_selftest_grow_limits; capacities 0 = default and only ever lowered, policies -1 = default).
        Called without arguments it clears every limit.  grow_counters() tells which were reached."""
        lim = _lib.GrowLimits(int(max_waves), int(pool_cap), int(max_pending), int(pstore_cap), int(retry_max_list),
                              int(retry_big_round), 1 if full_refresh else 0, 0)
        self._check(self._L.bs_selftest_grow_limits(self._h, C.byref(lim)))

    def selftest_scratch_guard(self, canary=True, poison=None):
        """Guard every following allocation of this context's scratch (bs_selftest_scratch_guard): a canary behind the
        requested bytes and, with poison = a byte value, that byte in front.  Only right after the context was made."""
        flags = (1 if canary else 0) | (2 if poison is not None else 0)
        self._check(self._L.bs_selftest_scratch_guard(self._h, flags, int(poison or 0)))

    @staticmethod
    def _scratch_slot(s) -> dict:
        return {"name": s.name.decode(), "address": s.address, "requested": s.requested, "guard": s.guard,
                "first_bad": s.first_bad, "last_bad": s.last_bad, "host": bool(s.host)}

    def selftest_scratch_check(self) -> dict:
        """Read every guard back (bs_selftest_scratch_check): n_guarded, bytes_requested, n_damaged and the first
        damaged buffers by bs_ctx member name, with the damaged range relative to the end of the request."""
        r = _lib.ScratchReport()
        self._check(self._L.bs_selftest_scratch_check(self._h, C.byref(r)))
        return {"n_guarded": r.n_guarded, "bytes_requested": r.bytes_requested, "n_damaged": r.n_damaged,
                "damaged": [self._scratch_slot(r.damaged[i]) for i in range(r.n_listed)]}

    def selftest_scratch_list(self) -> list:
        """Every buffer of this context allocated under the guard (bs_selftest_scratch_list), in bs_ctx order."""
        n = C.c_int64(0)
        self._check(self._L.bs_selftest_scratch_list(self._h, None, 0, C.byref(n)))
        slots = (_lib.ScratchSlot * max(n.value, 1))()
        self._check(self._L.bs_selftest_scratch_list(self._h, slots, n.value, C.byref(n)))
        return [self._scratch_slot(slots[i]) for i in range(n.value)]

    def grow_counters(self) -> dict:
        """bs_grow_counters of the last speculative region grow on this context (also after a failed one)."""
        g = _lib.GrowCounters()
        self._check(self._L.bs_get_grow_counters(self._h, C.byref(g)))
        return {k: getattr(g, k) for k, _ in _lib.GrowCounters._fields_}

    # ---- building blocks of the component-sharded stage 3 (device pointers) ----
    def cc_hook_dev(self, d_rows, d_gidx, m, k, d_parent, n_total) -> int:
        """One hooking step of the distributed union-find (bs_cc_hook_dev); returns the unions performed."""
        h = C.c_int64(0)
        self._check(self._L.bs_cc_hook_dev(self._h, d_rows or None, d_gidx or None, m, k, d_parent, n_total, C.byref(h)))
        return h.value

    def owner_fetch_dev(self, d_owner):
        """owner[p] of the last speculative grow on this context, in the caller's index order (-1: unlabelled)."""
        self._check(self._L.bs_owner_fetch_dev(self._h, d_owner))

    def plane_seeds_dev(self, d_seeds, cap) -> int:
        """Seeds of the committed planes of the last speculative grow (ascending) into d_seeds; returns their number."""
        npl = C.c_int32(0)
        self._check(self._L.bs_plane_seeds_dev(self._h, d_seeds or None, cap, C.byref(npl)))
        return npl.value

    def sync(self):
        self._check(self._L.bs_stream_sync(self._h))

    def labels_from_owner_dev(self, d_owner, n, d_seeds, n_seeds, d_plane_idx):
        self._check(self._L.bs_labels_from_owner_dev(self._h, d_owner or None, n, d_seeds or None, n_seeds, d_plane_idx or None))

    def remap_rows_dev(self, d_rows, n_rows, k, d_sorted_gidx, n, d_out) -> int:
        miss = C.c_int32(0)
        self._check(self._L.bs_remap_rows_dev(self._h, d_rows or None, n_rows, k, d_sorted_gidx or None, n, d_out or None,
                                              C.byref(miss)))
        return miss.value

    # ---- multi-GPU entry point of the C ABI (bs_segment_sharded) ----
    def segment_sharded(self, comm_ops, d_xyz, d_gidx, m, n_total, d_plane_idx, params, halo=0.0) -> dict:
        """ONE cloud spread over the ranks of `comm_ops` (a _lib.CommOps: bs_comm_rccl / bs_comm_local_create);
        this rank passes its m points (device pointers).  d_plane_idx [n_total] receives the labels of the whole
        cloud.  Returns bs_shard_info as a dict."""
        inf = _lib.ShardInfo()
        self._check(self._L.bs_segment_sharded(self._h, C.byref(comm_ops) if comm_ops is not None else None, d_xyz or None,
                                               d_gidx or None, m, n_total, C.byref(params), float(halo), d_plane_idx,
                                               C.byref(inf)))
        return {k: getattr(inf, k) for k, _ in _lib.ShardInfo._fields_}

    def sharded_planes_fetch(self):
        """The planes THIS rank grew in the last segment_sharded, with global ids and global point indices."""
        P = Planes()
        self._check(self._L.bs_sharded_planes_fetch(self._h, C.byref(P)))
        planes = _planes_to_list(P)
        self._L.bs_planes_free(C.byref(P))
        return planes

    def planes_fetch(self):
        P = Planes()
        self._check(self._L.bs_planes_fetch(self._h, C.byref(P)))
        planes = _planes_to_list(P)
        self._L.bs_planes_free(C.byref(P))
        return planes

    # ---- batches of independent tiles (bs_segment_batch) ----------------------
    def segment_batch(self, tiles, params: Params | None = None, shift_to_origin: bool = False):
        """Segment a list of independent int32 [n_t, 3] clouds in one device pass.  Returns one
        (neigh, normals, plane_idx, planes) per tile, each what segment() returns for that tile alone.
        shift_to_origin: move every tile to its own bounding-box origin first (TMC3.cpp:55-73 per tile)."""
        p = params or default_params()
        xyz, off = pack_tiles(tiles)
        if shift_to_origin:
            xyz = shift_tiles_to_origin(xyz, off)
        n, nt = len(xyz), len(off) - 1
        neigh = np.empty((n, p.k), dtype=np.int32)
        normals = np.empty((n, 3), dtype=np.float64)
        plane_idx = np.empty(n, dtype=np.int32)
        poff = np.empty(nt + 1, dtype=np.int32)
        P = Planes()
        self._batch_tiles = 0
        self._check(self._L.bs_segment_batch(self._h, xyz.ctypes.data, off.ctypes.data, nt, C.byref(p),
                                             neigh.ctypes.data, normals.ctypes.data, plane_idx.ctypes.data,
                                             C.byref(P), poff.ctypes.data))
        self._batch_tiles = nt
        planes = _planes_to_list(P)
        self._L.bs_planes_free(C.byref(P))
        return [(neigh[off[t]:off[t + 1]], normals[off[t]:off[t + 1]], plane_idx[off[t]:off[t + 1]],
                 planes[poff[t]:poff[t + 1]]) for t in range(nt)]

    def segment_batch_dev(self, d_xyz, tile_offset, d_plane_idx, params, d_neigh=0, d_normals=0):
        """Device form: d_xyz holds the concatenated tiles, tile_offset [n_tiles + 1] (host) delimits them; the plane
        records stay on the device until batch_planes_fetch()."""
        off = _tile_offsets(tile_offset)
        self._batch_tiles = 0
        self._check(self._L.bs_segment_batch_dev(self._h, d_xyz, off.ctypes.data, len(off) - 1, C.byref(params),
                                                 d_neigh or None, d_normals or None, d_plane_idx))
        self._batch_tiles = len(off) - 1

    def batch_planes_fetch(self):
        """The planes of the last batch on this context: one list per tile (ids from 1, tile-local point indices)."""
        nt = getattr(self, "_batch_tiles", 0)
        poff = np.zeros(nt + 1, dtype=np.int32)
        P = Planes()
        self._check(self._L.bs_batch_planes_fetch(self._h, C.byref(P), poff.ctypes.data if nt else None))
        planes = _planes_to_list(P)
        self._L.bs_planes_free(C.byref(P))
        return [planes[poff[t]:poff[t + 1]] for t in range(nt)]

    def shift_tiles_to_origin_dev(self, d_xyz, tile_offset):
        """bs_shift_to_origin_dev for every tile of the concatenation separately; returns the minima [n_tiles, 3]."""
        off = _tile_offsets(tile_offset)
        mn = np.zeros((len(off) - 1, 3), dtype=np.int32)
        self._check(self._L.bs_shift_tiles_to_origin_dev(self._h, d_xyz, off.ctypes.data, len(off) - 1,
                                                         mn.ctypes.data))
        return mn

    # ---- batches of rasters and footprints (bs_grid_picture_batch, bs_footprints_batch) ----
    def tile_boxes_dev(self, d_xyz, tile_offset):
        """Per-tile {min x, y, z, max x, y, z} of a device-resident concatenation: int32 [n_tiles, 6]."""
        off = _tile_offsets(tile_offset)
        box = np.zeros((len(off) - 1, 6), dtype=np.int32)
        self._check(self._L.bs_tile_boxes_dev(self._h, d_xyz, off.ctypes.data, len(off) - 1, box.ctypes.data))
        return box

    def grid_picture_batch(self, tiles, extents=None, bin=100, bin_height=1000, shift_to_origin=False):
        """grid_picture for every tile of a list of int32 [n_t, 3] clouds, in one device pass.  Returns one
        (image [height][width][3] f64, ground_th) per tile, each what grid_picture returns for that tile alone.
        extents: [n_tiles, 3] (default: each tile's maximum); shift_to_origin: move every tile to its own
        bounding-box origin first."""
        xyz, off = pack_tiles(tiles)
        if shift_to_origin:
            xyz = shift_tiles_to_origin(xyz, off)
        nt = len(off) - 1
        ext = _tile_extents(np.maximum.reduceat(xyz, off[:-1], axis=0) if extents is None else extents, nt)
        w, h, po = grid_dims_batch(ext, bin)
        img = np.empty(3 * int(po[-1]), dtype=np.float64)
        th = np.empty(nt, dtype=np.float64)
        self._check(self._L.bs_grid_picture_batch(self._h, xyz.ctypes.data, off.ctypes.data, nt, ext.ctypes.data, bin,
                                                  bin_height, img.ctypes.data, th.ctypes.data))
        return [(img[3 * po[t]:3 * po[t + 1]].reshape(h[t], w[t], 3), float(th[t])) for t in range(nt)]

    def grid_picture_batch_dev(self, d_xyz, tile_offset, extents, d_image, bin=100, bin_height=1000):
        """Device form: d_xyz holds the shifted tiles, d_image receives the images at grid_dims_batch's pixel
        offsets (device pointers, ints).  Returns the ground thresholds [n_tiles]."""
        off = _tile_offsets(tile_offset)
        nt = len(off) - 1
        ext = _tile_extents(extents, nt)
        th = np.empty(nt, dtype=np.float64)
        self._check(self._L.bs_grid_picture_batch_dev(self._h, d_xyz, off.ctypes.data, nt, ext.ctypes.data, bin,
                                                      bin_height, d_image, th.ctypes.data))
        return th

    def footprints_batch(self, images, threshold=10, kernel_size=5, iterations=2, return_mask=False):
        """footprints for every [height][width][3] f64 raster of a list, in one device pass.  Returns one
        Footprints per tile (with that tile's width and height; info: the whole pass) and, with return_mask, the
        list of closed masks as well."""
        if isinstance(images, np.ndarray) or not hasattr(images, "__len__") or len(images) == 0:
            raise ValueError("images must be a non-empty list of [height][width][3] arrays")
        imgs = []
        for t, a in enumerate(images):
            a = np.asarray(a, dtype=np.float64)
            if a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"footprints_batch: tile {t}: image must be [height][width][3], got {a.shape}")
            imgs.append(a)
        nt = len(imgs)
        w = np.array([a.shape[1] for a in imgs], dtype=np.int32)
        h = np.array([a.shape[0] for a in imgs], dtype=np.int32)
        po = np.zeros(nt + 1, dtype=np.int64)
        po[1:] = np.cumsum(w.astype(np.int64) * h)
        flat = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in imgs]))
        mask = np.empty(int(po[-1]), dtype=np.uint8) if return_mask else None
        out, inf, co = Contours(), FootprintInfo(), np.zeros(nt + 1, dtype=np.int32)
        self._check(self._L.bs_footprints_batch(self._h, flat.ctypes.data, w.ctypes.data, h.ctypes.data, nt, threshold,
                                                kernel_size, iterations, _ptr(mask), C.byref(out), co.ctypes.data,
                                                C.byref(inf)))
        fps = _take_contours_batch(self._L, out, inf, co, w, h)
        if return_mask:
            return fps, [mask[po[t]:po[t + 1]].reshape(h[t], w[t]) for t in range(nt)]
        return fps

    def footprints_batch_dev(self, d_image, widths, heights, threshold=10, kernel_size=5, iterations=2, d_mask=0):
        """Device form: d_image holds the tile images at grid_dims_batch's pixel offsets, d_mask (optional) receives
        the closed masks at the same offsets (device pointers, ints).  Returns one Footprints per tile."""
        w = np.ascontiguousarray(widths, dtype=np.int32)
        h = np.ascontiguousarray(heights, dtype=np.int32)
        if w.ndim != 1 or w.shape != h.shape or len(w) == 0:
            raise ValueError("widths and heights must be 1-D arrays of the same length >= 1")
        out, inf, co = Contours(), FootprintInfo(), np.zeros(len(w) + 1, dtype=np.int32)
        self._check(self._L.bs_footprints_batch_dev(self._h, d_image or None, w.ctypes.data, h.ctypes.data, len(w),
                                                    threshold, kernel_size, iterations, d_mask or None, C.byref(out),
                                                    co.ctypes.data, C.byref(inf)))
        return _take_contours_batch(self._L, out, inf, co, w, h)

    # ---- buildings: footprints joined with the points and the planes (bs_building_map, bs_assign_buildings, ...) ----
    def building_map(self, mask):
        """Building map of a closed [height][width] mask (non-zero = foreground, e.g. footprints(return_mask=True)):
        returns (map int32 [height][width]: building of every pixel or -1, Buildings).  Building c is contour c of
        footprints() on the same mask."""
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        if m.ndim != 2:
            raise ValueError("building_map: mask must be [height][width]")
        h, w = m.shape
        bmap = np.empty((h, w), dtype=np.int32)
        out = _lib.Buildings()
        self._check(self._L.bs_building_map(self._h, m.ctypes.data, w, h, bmap.ctypes.data, C.byref(out)))
        return bmap, _take_buildings(self._L, out)

    def building_map_dev(self, d_mask, width, height, d_map):
        """Device-resident variant: d_mask ([height][width] uint8) and d_map ([height][width] int32, out) are device
        pointers (ints); the per-building figures come back in host memory."""
        out = _lib.Buildings()
        self._check(self._L.bs_building_map_dev(self._h, d_mask or None, width, height, d_map or None, C.byref(out)))
        return _take_buildings(self._L, out)

    def assign_buildings(self, xyz, bmap, buildings, bin=100, ground_th=0.0):
        """building_idx int32 [n] of a cloud shifted to its origin: the building of every point's base pixel
        (x / bin, y / bin) in bmap, -1 outside every building.  Fills the point figures of `buildings` (the object
        building_map returned for bmap): n_points, n_above, z_min, z_max, z_sum over the points with
        !(z < ground_th)."""
        xyz = _points("assign_buildings", xyz)
        bmap = np.ascontiguousarray(bmap, dtype=np.int32)
        h, w = bmap.shape
        bidx = np.empty(len(xyz), dtype=np.int32)
        st = _buildings_struct(buildings)
        self._check(self._L.bs_assign_buildings(self._h, xyz.ctypes.data, len(xyz), bin, float(ground_th),
                                                bmap.ctypes.data, w, h, bidx.ctypes.data, C.byref(st)))
        buildings.info["ms_assign"] = st.ms_assign
        return bidx

    def assign_buildings_dev(self, d_xyz, n, d_map, buildings, d_building_idx, bin=100, ground_th=0.0):
        """Device-resident variant: d_xyz, d_map ([height][width] of `buildings`) and d_building_idx (int32 [n], out)
        are device pointers (ints)."""
        st = _buildings_struct(buildings)
        self._check(self._L.bs_assign_buildings_dev(self._h, d_xyz or None, n, bin, float(ground_th), d_map or None,
                                                    buildings.width, buildings.height, d_building_idx or None,
                                                    C.byref(st)))
        buildings.info["ms_assign"] = st.ms_assign

    def plane_buildings(self, plane_idx, building_idx, n_planes, n_buildings):
        """Votes of the planes 1 .. n_planes for the buildings, over the point labels: returns PlaneVotes (arrays
        [n_planes], entry p - 1 = plane p)."""
        pi = np.ascontiguousarray(plane_idx, dtype=np.int32)
        bi = np.ascontiguousarray(building_idx, dtype=np.int32)
        if pi.shape != bi.shape or pi.ndim != 1:
            raise ValueError("plane_idx and building_idx must be 1-D arrays of the same length")
        return self._votes(self._L.bs_plane_buildings, pi.ctypes.data, bi.ctypes.data, len(pi), n_planes, n_buildings)

    def plane_buildings_dev(self, d_plane_idx, d_building_idx, n, n_planes, n_buildings):
        """Device-resident variant: the two label arrays are device pointers (ints)."""
        return self._votes(self._L.bs_plane_buildings_dev, d_plane_idx or None, d_building_idx or None, n, n_planes,
                           n_buildings)

    def _votes(self, fn, p_plane, p_bidx, n, n_planes, n_buildings):
        m = max(int(n_planes), 0)
        pb = np.full(m, -1, dtype=np.int32)
        vin, vtot, vout = (np.zeros(m, dtype=np.int64) for _ in range(3))
        self._check(fn(self._h, p_plane, p_bidx, n, n_planes, n_buildings, pb.ctypes.data, vin.ctypes.data,
                       vtot.ctypes.data, vout.ctypes.data))
        return PlaneVotes(pb, vin, vtot, vout)

    def buildings(self, xyz, plane_idx=None, n_planes=0, bin=100, bin_height=1000, threshold=10, kernel_size=5,
                  iterations=2, ground=None, evidence=None):
        """The whole 2-D branch for a cloud shifted to its origin: raster -> footprints (with the closed mask) ->
        building map -> point assignment -> plane votes (when plane_idx, the labels of segment(), is given).
        Returns (Footprints, Buildings); the Buildings carry map, building_idx, ground_th and votes.  ground: a dict of
        the parameters of ground() ({} for its defaults): the stage runs first, the raster and the assignment of this call
        measure "above ground" against its dtm (set_ground_model; the context's own model is restored afterwards), and
        the Ground is returned as a third value.  evidence: a dict of evidence_params() ({} for its defaults; it needs
        plane_idx and n_planes): plane_fit -> plane_quality -> roof_evidence run after the raster, under the ground model
        if one was asked for, the footprints of this call are taken under its keep image (set_footprint_screen; the
        context's own screen is restored afterwards), and the RoofEvidence is returned as the last value."""
        xyz = np.ascontiguousarray(xyz, dtype=np.int32)
        if evidence is not None and plane_idx is None:
            raise ValueError("buildings: evidence needs plane_idx, the labels of segment()")
        if ground is not None:
            g = self.ground(xyz, points=False, **ground)
            with self._ground_model(g):
                out = self.buildings(xyz, plane_idx, n_planes, bin=bin, bin_height=bin_height, threshold=threshold,
                                     kernel_size=kernel_size, iterations=iterations, evidence=evidence)
            return out[:2] + (g,) + out[2:]
        img, th = self.grid_picture(xyz, bin=bin, bin_height=bin_height)
        ev = None
        if evidence is not None:
            ev = self._evidence(xyz, plane_idx, n_planes, bin, th, evidence)
        with self._footprint_screen(ev.keep) if ev is not None else nullcontext():
            fp, mask = self.footprints(img, threshold=threshold, kernel_size=kernel_size, iterations=iterations,
                                       return_mask=True)
        bmap, b = self.building_map(mask)
        b.map, b.ground_th = bmap, th
        b.building_idx = self.assign_buildings(xyz, bmap, b, bin=bin, ground_th=th)
        if plane_idx is not None:
            b.votes = self.plane_buildings(plane_idx, b.building_idx, n_planes, b.n_buildings)
        return (fp, b) if ev is None else (fp, b, ev)

    # ---- roofs: the plane over every pixel of a building and its height there (bs_roofs, include/bs_api.h) ----------
    def roofs(self, xyz, bmap, plane_idx, home, normal, center, bin=100, ground_th=0.0, min_votes=1, support=True,
              height=True):
        """Roof plane of every building pixel for a cloud shifted to its origin: vote of the counting points per pixel,
        fill in synchronous rounds, per-plane figures and heights.  bmap is the building map, plane_idx the labels,
        home / normal / center the per-plane tables (entry p - 1 is plane p; home from roof_homes).  Returns Roofs with
        roof, support and height [height][width] int32 (support / height None when switched off)."""
        xyz = _points("roofs", xyz)
        bmap = np.ascontiguousarray(bmap, dtype=np.int32)
        if bmap.ndim != 2:
            raise ValueError("roofs: bmap must be [height][width]")
        pi = _point_labels("roofs", "plane_idx", plane_idx, xyz)
        h, w = bmap.shape
        tabs = _roof_tables(home, normal, center)
        roof = np.empty((h, w), dtype=np.int32)
        sup = np.empty((h, w), dtype=np.int32) if support else None
        hgt = np.empty((h, w), dtype=np.int32) if height else None
        out = _lib.Roofs()
        self._check(self._L.bs_roofs(self._h, xyz.ctypes.data, len(xyz), bin, float(ground_th), bmap.ctypes.data, w, h,
                                     pi.ctypes.data, len(tabs[0]), *[t.ctypes.data for t in tabs], min_votes,
                                     roof.ctypes.data, _ptr(sup), _ptr(hgt), C.byref(out)))
        return _take_roofs(self._L, out, roof, sup, hgt, tabs, bin)

    def roofs_dev(self, d_xyz, n, d_map, width, height, d_plane_idx, home, normal, center, d_roof, d_support=0,
                  d_height=0, bin=100, ground_th=0.0, min_votes=1, n_planes=None):
        """Device-resident variant: d_xyz, d_map, d_plane_idx, d_roof and the optional d_support / d_height are device
        pointers (ints); the tables stay host arrays.  The Roofs that comes back holds the figures only."""
        tabs = _roof_tables(home, normal, center)
        out = _lib.Roofs()
        self._check(self._L.bs_roofs_dev(self._h, d_xyz or None, n, bin, float(ground_th), d_map or None, width, height,
                                         d_plane_idx or None, len(tabs[0]) if n_planes is None else n_planes,
                                         *[t.ctypes.data for t in tabs], min_votes, d_roof or None, d_support or None,
                                         d_height or None, C.byref(out)))
        return _take_roofs(self._L, out, None, None, None, tabs, bin)

    # ---- plane fit: exact centroid, least-squares normal and residuals per plane (bs_plane_fit, include/bs_api.h) ------
    def plane_fit(self, xyz, plane_idx, n_planes, residuals=False):
        """Refit the planes 1 .. n_planes from the points that carry their label.  Returns PlaneFits (arrays [n_planes],
        entry p - 1 = plane p); with residuals=True its `residual` is the [n] int32 truncated distance of every point to
        its fitted plane (INT32_MIN for the points of no fitted plane)."""
        xyz = _points("plane_fit", xyz)
        pi = _point_labels("plane_fit", "plane_idx", plane_idx, xyz)
        res = np.empty(len(xyz), dtype=np.int32) if residuals else None
        out = _lib.PlaneFits()
        self._check(self._L.bs_plane_fit(self._h, xyz.ctypes.data, len(xyz), pi.ctypes.data, n_planes, _ptr(res),
                                         C.byref(out)))
        return _take_fits(self._L, out, res)

    def plane_fit_dev(self, d_xyz, n, d_plane_idx, n_planes, d_residual=0):
        """Device-resident variant: d_xyz, d_plane_idx and the optional d_residual [n] int32 are device pointers (ints)."""
        out = _lib.PlaneFits()
        self._check(self._L.bs_plane_fit_dev(self._h, d_xyz or None, n, d_plane_idx or None, n_planes, d_residual or None,
                                             C.byref(out)))
        return _take_fits(self._L, out, None)

    def roof_model(self, xyz, plane_idx, planes, bin=100, bin_height=1000, threshold=10, kernel_size=5, iterations=2,
                   min_normal_z=0.5, min_votes=1, refit=False, ground=None, evidence=None):
        """buildings() -> roof_homes -> roofs for a cloud shifted to its origin, its labels and the planes of segment().
        Returns (Footprints, Buildings, Roofs); the Roofs carry home, normal, center and bin for write_roofs_obj.
        refit=True: plane_fit() after buildings(), and homes and roofs from the refitted normal / center tables (which
        the Roofs then carry, with the PlaneFits as `fit`).  ground: as for buildings(); the roofs of this call count their
        points against the same dtm, and the Ground is returned as a fourth value.  evidence: as for buildings(); the
        RoofEvidence is returned as the last value."""
        if ground is not None:
            g = self.ground(xyz, points=False, **ground)
            with self._ground_model(g):
                out = self.roof_model(xyz, plane_idx, planes, bin=bin, bin_height=bin_height, threshold=threshold,
                                      kernel_size=kernel_size, iterations=iterations, min_normal_z=min_normal_z,
                                      min_votes=min_votes, refit=refit, evidence=evidence)
            return out[:3] + (g,) + out[3:]
        n_planes = len(planes)
        if [p.id for p in planes] != list(range(1, n_planes + 1)):
            raise ValueError("roof_model: planes must be the planes 1 .. n of segment(), in order")
        normal = np.array([p.normal for p in planes], dtype=np.float64).reshape(n_planes, 3)
        center = np.array([p.center for p in planes], dtype=np.int32).reshape(n_planes, 3)
        fp, b, *ev = self.buildings(xyz, plane_idx, n_planes, bin=bin, bin_height=bin_height, threshold=threshold,
                                    kernel_size=kernel_size, iterations=iterations, evidence=evidence)
        fit = None
        if refit:
            fit = self.plane_fit(xyz, plane_idx, n_planes)
            normal, center = plane_fit_apply(fit, normal, center)
        home = roof_homes(normal, b.votes.plane_building, b.votes.votes_in, b.votes.votes_total, min_normal_z)
        r = self.roofs(xyz, b.map, plane_idx, home, normal, center, bin=bin, ground_th=b.ground_th, min_votes=min_votes)
        r.fit = fit
        return (fp, b, r) + tuple(ev)

    # ---- solids: a closed oriented mesh per building from the roof image (bs_solids, include/bs_api.h) ---------------
    def solids(self, bmap, roofs, buildings=None, base_z=None, flat=None, top=True):
        """Roof, walls and floor of every building as one closed mesh.  bmap is the building map, `roofs` the Roofs of
        roofs() on it (its roof image, plane tables, z_min / z_max and bin are used).  base_z defaults to
        (int) buildings.ground_th; flat [n_buildings], the top of the unroofed pixels, to z_sum / n_above truncated
        (write_buildings_obj's top) and to base_z where n_above == 0.  Returns Solids."""
        bmap, roof, base_z, flat, tabs = _solid_inputs("solids", bmap, roofs, buildings, base_z, flat)
        h, w = bmap.shape
        timg = np.empty((h, w, 4), dtype=np.int32) if top else None
        out = _lib.Solids()
        self._check(self._L.bs_solids(self._h, bmap.ctypes.data, roof.ctypes.data, w, h, len(flat), len(tabs[0]),
                                      *[t.ctypes.data for t in tabs], int(roofs.bin), base_z, _ptr0(flat), _ptr(timg),
                                      C.byref(out)))
        s = _take_solids(self._L, out, timg, True)
        s.base = self.building_bases()
        return s

    def solids_dev(self, d_map, d_roof, width, height, normal, center, z_min, z_max, bin, base_z, flat, d_top=0):
        """Device-resident count (bs_solids_count_dev): d_map, d_roof and the optional d_top ([height][width][4] int32)
        are device pointers (ints), the tables host arrays; len(flat) is n_buildings.  Returns Solids with the figures
        and the sizes n_vertices / n_faces / n_indices of the buffers solids_emit_dev fills."""
        tabs = _solid_tables(normal, center, z_min, z_max)
        flat = np.ascontiguousarray(flat, dtype=np.int32).reshape(-1)
        out = _lib.Solids()
        self._check(self._L.bs_solids_count_dev(self._h, d_map or None, d_roof or None, width, height, len(flat),
                                                len(tabs[0]), *[t.ctypes.data for t in tabs], int(bin), int(base_z),
                                                _ptr0(flat), d_top or None, C.byref(out)))
        s = _take_solids(self._L, out, None, False)
        s.base = self.building_bases()
        return s

    def solids_emit_dev(self, d_vertex, d_face_offset, d_face_index, d_face_building, d_face_kind):
        """The mesh of the last solids_dev on this context into device buffers (ints) of exactly its sizes."""
        self._check(self._L.bs_solids_emit_dev(self._h, d_vertex or None, d_face_offset or None, d_face_index or None,
                                               d_face_building or None, d_face_kind or None))

    def solid_model(self, xyz, plane_idx, planes, bin=100, bin_height=1000, threshold=10, kernel_size=5, iterations=2,
                    min_normal_z=0.5, min_votes=1, refit=False, base_z=None, flat=None, generalise=None, terrain=None,
                    ground=None, evidence=None):
        """roof_model() followed by solids(): returns (Footprints, Buildings, Roofs, Solids).  generalise: a dict of the
        parameters of generalise_roofs() (min_pixels, merge_flat, step_tol, bend_tol, max_rounds); the Roofs returned are
        then the generalised ones and the Solids theirs.  terrain: a dict of the parameters of terrain() (ring, q,
        min_ground; {} for its defaults): the stage runs after the buildings with fallback_z = int(ground_th), its `ground`
        is the base of every building for the generalisation and the solids (flat defaults to it where a building has no
        point above ground), the context's own table is restored afterwards, and the Terrain is returned as a fifth
        value.  ground: as for roof_model(); the Ground is returned as an additional value after these.  evidence: as for
        buildings(); the RoofEvidence is returned as the last value."""
        if ground is not None:
            g = self.ground(xyz, points=False, **ground)
            with self._ground_model(g):
                out = self.solid_model(xyz, plane_idx, planes, bin=bin, bin_height=bin_height, threshold=threshold,
                                       kernel_size=kernel_size, iterations=iterations, min_normal_z=min_normal_z,
                                       min_votes=min_votes, refit=refit, base_z=base_z, flat=flat, generalise=generalise,
                                       terrain=terrain, evidence=evidence)
            return (out + (g,)) if evidence is None else (out[:-1] + (g, out[-1]))
        fp, b, r, *ev = self.roof_model(xyz, plane_idx, planes, bin=bin, bin_height=bin_height, threshold=threshold,
                                        kernel_size=kernel_size, iterations=iterations, min_normal_z=min_normal_z,
                                        min_votes=min_votes, refit=refit, evidence=evidence)
        ev = tuple(ev)
        if terrain is None:
            if generalise is not None:
                r = self.generalise_roofs(b.map, r, b, base_z=base_z, flat=flat, **generalise).roofs
            return (fp, b, r, self.solids(b.map, r, b, base_z=base_z, flat=flat)) + ev
        t = self.terrain(xyz, b.map, b, bin=bin, fallback_z=int(b.ground_th), **terrain)
        if flat is None:
            scalar, flat = _solid_defaults(b, base_z, None)
            flat = np.where(np.asarray(b.n_above) > 0, flat, t.ground).astype(np.int32)
        with self._bases(t.ground if b.n_buildings else None):
            if generalise is not None:
                r = self.generalise_roofs(b.map, r, b, base_z=base_z, flat=flat, **generalise).roofs
            s = self.solids(b.map, r, b, base_z=base_z, flat=flat)
        return (fp, b, r, s, t) + ev

    # ---- roof generalisation: small and coplanar facets merged (bs_roof_generalise, include/bs_api.h) ------------------
    def generalise_roofs(self, bmap, roofs, buildings=None, base_z=None, flat=None, min_pixels=0, merge_flat=False,
                         step_tol=200, bend_tol=0, max_rounds=64):
        """Merge every roof facet with fewer than min_pixels pixels, and (merge_flat) every facet across a FLAT edge, into
        its highest-ranking neighbour with the longest common border, round by round until nothing moves (or max_rounds
        rounds were applied).  The arguments before min_pixels are those of solids().  Returns RoofGeneralise: the
        figures, .roof (the new roof image) and .roofs (a Roofs every later stage accepts)."""
        bmap, roof, base_z, flat, tabs = _solid_inputs("generalise_roofs", bmap, roofs, buildings, base_z, flat)
        h, w = bmap.shape
        par = _lib.RoofGeneraliseParams(int(min_pixels), int(merge_flat), int(step_tol), int(bend_tol), int(max_rounds))
        new = np.empty((h, w), dtype=np.int32)
        out = _lib.RoofGeneralise()
        self._check(self._L.bs_roof_generalise(self._h, bmap.ctypes.data, roof.ctypes.data, w, h, len(flat), len(tabs[0]),
                                               *[t.ctypes.data for t in tabs], int(roofs.bin), base_z, _ptr0(flat),
                                               C.byref(par), new.ctypes.data, C.byref(out)))
        g = _take_roof_generalise(self._L, out, new)
        g.roofs = copy.copy(roofs)  # the tables, z_min / z_max and bin stay
        g.roofs.roof, g.roofs.pixels, g.roofs.support, g.roofs.height = new, g.plane_pixels_out[1:].copy(), None, None
        return g

    def generalise_roofs_dev(self, d_map, d_roof, width, height, normal, center, z_min, z_max, bin, base_z, flat, d_roof_out,
                             min_pixels=0, merge_flat=False, step_tol=200, bend_tol=0, max_rounds=64):
        """Device-resident form (bs_roof_generalise_dev): d_map, d_roof and d_roof_out ([height][width] int32, written; it
        may be d_roof) are device pointers (ints), the tables host arrays; len(flat) is n_buildings.  Returns
        RoofGeneralise with roof and roofs None."""
        tabs = _solid_tables(normal, center, z_min, z_max)
        flat = np.ascontiguousarray(flat, dtype=np.int32).reshape(-1)
        par = _lib.RoofGeneraliseParams(int(min_pixels), int(merge_flat), int(step_tol), int(bend_tol), int(max_rounds))
        out = _lib.RoofGeneralise()
        self._check(self._L.bs_roof_generalise_dev(self._h, d_map or None, d_roof or None, width, height, len(flat),
                                                   len(tabs[0]), *[t.ctypes.data for t in tabs], int(bin), int(base_z),
                                                   _ptr0(flat), C.byref(par), d_roof_out or None, C.byref(out)))
        return _take_roof_generalise(self._L, out, None)

    # ---- roof facets and the edges between them (bs_roof_facets, include/bs_api.h) -------------------------------------
    def roof_facets(self, bmap, roof, top, n_buildings=None, n_planes=None):
        """The roof facets of every building (4-connected pixels of one building under one plane) and the edges between
        them.  bmap and roof are [height][width], top [height][width][4] as Solids.top.  n_buildings defaults to
        bmap.max() + 1, n_planes to max(roof.max(), 0).  Returns RoofFacets."""
        bmap = np.ascontiguousarray(bmap, dtype=np.int32)
        roof = np.ascontiguousarray(roof, dtype=np.int32)
        top = np.ascontiguousarray(top, dtype=np.int32)
        if bmap.ndim != 2 or bmap.size == 0 or roof.shape != bmap.shape or top.shape != bmap.shape + (4,):
            raise ValueError("roof_facets: bmap and roof must be [height][width] and top [height][width][4]")
        h, w = bmap.shape
        nb = max(int(bmap.max()) + 1, 0) if n_buildings is None else int(n_buildings)
        npl = max(int(roof.max()), 0) if n_planes is None else int(n_planes)
        facet = np.empty((h, w), dtype=np.int32)
        out = _lib.RoofFacets()
        self._check(self._L.bs_roof_facets(self._h, bmap.ctypes.data, roof.ctypes.data, top.ctypes.data, w, h, nb, npl,
                                           facet.ctypes.data, C.byref(out)))
        return _take_roof_facets(self._L, out, facet)

    def roof_facets_dev(self, d_map, d_roof, d_top, width, height, n_buildings, n_planes, d_facet):
        """Device-resident form (bs_roof_facets_dev): the four images are device pointers (ints), d_facet
        [height][width] int32 is written.  Returns RoofFacets with facet None."""
        out = _lib.RoofFacets()
        self._check(self._L.bs_roof_facets_dev(self._h, d_map or None, d_roof or None, d_top or None, width, height,
                                               int(n_buildings), int(n_planes), d_facet or None, C.byref(out)))
        return _take_roof_facets(self._L, out, None)

    def roof_structure(self, bmap, roofs, solids):
        """roof_facets() from the Roofs of roofs() and the Solids of solids() on the same map."""
        _has_top("roof_structure", solids)
        _host_image("roof_structure", roofs.roof, "roof", "roof_facets_dev")
        return self.roof_facets(bmap, roofs.roof, solids.top, n_buildings=solids.n_buildings, n_planes=len(roofs.z_min))

    # ---- facet outlines: polygon rings with holes per label (bs_facet_outlines, include/bs_api.h) ------------------------
    def facet_outlines(self, label, top=None, n_labels=None):
        """Every label of a label image ([height][width], negative = outside) as polygon rings with holes; with top
        ([height][width][4] as Solids.top) every vertex carries a Z.  n_labels defaults to label.max() + 1.  Returns
        Outlines."""
        label, top, h, w, nl = _label_top("facet_outlines", label, top, n_labels)
        out = _lib.Outlines()
        self._check(self._L.bs_facet_outlines(self._h, label.ctypes.data, _ptr(top), w, h, nl, C.byref(out)))
        return _take_outlines(self._L, out, True)

    def facet_outlines_dev(self, d_label, d_top, width, height, n_labels):
        """Device-resident count (bs_facet_outlines_count_dev): d_label and d_top (0: no Z) are device pointers (ints).
        Returns Outlines with xy and z None and the size n_vertices of the buffers facet_outlines_emit_dev fills."""
        out = _lib.Outlines()
        self._check(self._L.bs_facet_outlines_count_dev(self._h, d_label or None, d_top or None, width, height,
                                                        int(n_labels), C.byref(out)))
        return _take_outlines(self._L, out, False)

    def facet_outlines_emit_dev(self, d_xy, d_z=0):
        """The vertices of the last facet_outlines_dev on this context into device buffers (ints) of exactly its sizes:
        d_xy [n_vertices][2], d_z [n_vertices] (0 iff the count had no top)."""
        self._check(self._L.bs_facet_outlines_emit_dev(self._h, d_xy or None, d_z or None))

    def roof_outlines(self, roof_facets, solids):
        """facet_outlines() of the facet image of roof_facets() / roof_structure() with the tops of solids()."""
        _facet_and_top("roof_outlines", roof_facets, solids, "facet_outlines_dev")
        return self.facet_outlines(roof_facets.facet, solids.top, n_labels=roof_facets.n_facets)

    # ---- simplified outlines: shared arcs, exact Douglas-Peucker (bs_simple_outlines, include/bs_api.h) ----------------
    def simplified_outlines(self, label, top=None, n_labels=None, num=0, den=1):
        """The outlines of facet_outlines() cut into the arcs that two labels share, every arc simplified by an exact
        Douglas-Peucker with the tolerance tol2 = num / den in lattice units squared (simplify_tolerance()).  Returns
        (SimpleOutlines, the plain Outlines without vertices)."""
        label, top, h, w, nl = _label_top("simplified_outlines", label, top, n_labels)
        out, plain = _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_simple_outlines(self._h, label.ctypes.data, _ptr(top), w, h, nl, int(num), int(den),
                                               C.byref(out), C.byref(plain)))
        return _take_chain(self._L, (_take_simple_outlines, out, True), (_take_outlines, plain, False))

    def simplified_outlines_dev(self, d_label, d_top, width, height, n_labels, num=0, den=1):
        """Device-resident count (bs_simple_outlines_count_dev): d_label and d_top (0: no Z) are device pointers (ints).
        Returns (SimpleOutlines with the vertex arrays None and the size n_svertices of the buffers
        simplified_outlines_emit_dev fills, the plain Outlines without vertices)."""
        out, plain = _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_simple_outlines_count_dev(self._h, d_label or None, d_top or None, width, height,
                                                         int(n_labels), int(num), int(den), C.byref(out), C.byref(plain)))
        return _take_chain(self._L, (_take_simple_outlines, out, False), (_take_outlines, plain, False))

    def simplified_outlines_emit_dev(self, d_sxy, d_sz, d_right, d_flag):
        """The kept vertices of the last simplified_outlines_dev on this context into device buffers (ints) of exactly
        its sizes: d_sxy [n_svertices][2], d_sz [n_svertices] (0 iff the count had no top), d_right [n_svertices] int32,
        d_flag [n_svertices] uint8."""
        self._check(self._L.bs_simple_outlines_emit_dev(self._h, d_sxy or None, d_sz or None, d_right or None, d_flag or None))

    def roof_polygons(self, roof_facets, solids, tolerance_mm=0, bin=None, clean=False, sweeps=None):
        """simplified_outlines() of the facet image of roof_facets() / roof_structure() with the tops of solids(), at a
        tolerance in millimetres (bin: the pixel edge, by default the Solids').  clean=True: clean_outlines() instead --
        polygons whose segments meet only in shared end points -- as (CleanOutlines, the plain Outlines); sweeps: the sweep
        mode of that clean count (set_outline_sweeps), None = the context's."""
        _facet_and_top("roof_polygons", roof_facets, solids, "simplified_outlines_dev")
        num, den = simplify_tolerance(tolerance_mm, solids.bin if bin is None else bin)
        if clean:
            c, _, plain = self.clean_outlines(roof_facets.facet, solids.top, n_labels=roof_facets.n_facets, num=num, den=den,
                                              sweeps=sweeps)
            return c, plain
        return self.simplified_outlines(roof_facets.facet, solids.top, n_labels=roof_facets.n_facets, num=num, den=den)

    # ---- clean outlines: conflicts between simplified segments found and repaired (bs_clean_outlines, include/bs_api.h) --
    def set_outline_sweeps(self, mode):
        """The sweep mode of every clean count on this context (bs_set_outline_sweeps): 0 off (the default), 1 report,
        2 repair -- segments whose chord passes over a whole ring without touching it are marked and repaired too."""
        self._check(self._L.bs_set_outline_sweeps(self._h, int(mode)))
        self._sweeps_mode = int(mode)

    def outline_sweeps(self):
        """The figures of the sweep detection of the last clean count on this context (bs_get_outline_sweeps)."""
        out = _lib.OutlineSweeps()
        self._check(self._L.bs_get_outline_sweeps(self._h, C.byref(out)))
        return OutlineSweeps(mode=out.mode, wave_cap=out.wave_cap, ms_sweep=out.ms_sweep,
                             **{k: getattr(out, k) for k in _lib.SWEEP_FIGURES})

    @contextmanager
    def _sweeps(self, mode):
        """the sweep mode for one call (None: the context's), the previous one restored behind it"""
        if mode is None:
            yield
            return
        prev = getattr(self, "_sweeps_mode", 0)
        self.set_outline_sweeps(mode)
        try:
            yield
        finally:
            self.set_outline_sweeps(prev)

    def clean_outlines(self, label, top=None, n_labels=None, num=0, den=1, max_rounds=-1, cell_log2=0, sweeps=None):
        """The simplified outlines with every conflict between kept segments (cross, touch, overlap) repaired by keeping
        further nodes.  max_rounds < 0: until clean; 0: check only (s_flag bit 3 and n_marked_first report the conflicts);
        > 0: a cap.  cell_log2: the broad-phase cell edge, 0 = the default.  sweeps: the sweep mode of this call
        (set_outline_sweeps), None = the context's.  Returns (CleanOutlines, the SimpleOutlines without vertices, the plain
        Outlines without vertices)."""
        label, top, h, w, nl = _label_top("clean_outlines", label, top, n_labels)
        out, simple, plain = _lib.CleanOutlines(), _lib.SimpleOutlines(), _lib.Outlines()
        with self._sweeps(sweeps):
            self._check(self._L.bs_clean_outlines(self._h, label.ctypes.data, _ptr(top), w, h, nl, int(num), int(den),
                                                  int(max_rounds), int(cell_log2), C.byref(out), C.byref(simple),
                                                  C.byref(plain)))
        return _take_chain(self._L, (_take_clean_outlines, out, True), (_take_simple_outlines, simple, False),
                           (_take_outlines, plain, False))

    def clean_outlines_dev(self, d_label, d_top, width, height, n_labels, num=0, den=1, max_rounds=-1, cell_log2=0,
                           sweeps=None):
        """Device-resident count (bs_clean_outlines_count_dev): d_label and d_top (0: no Z) are device pointers (ints).
        sweeps as clean_outlines.  Returns (CleanOutlines with the vertex arrays None, SimpleOutlines, Outlines)."""
        out, simple, plain = _lib.CleanOutlines(), _lib.SimpleOutlines(), _lib.Outlines()
        with self._sweeps(sweeps):
            self._check(self._L.bs_clean_outlines_count_dev(self._h, d_label or None, d_top or None, width, height,
                                                            int(n_labels), int(num), int(den), int(max_rounds),
                                                            int(cell_log2), C.byref(out), C.byref(simple), C.byref(plain)))
        return _take_chain(self._L, (_take_clean_outlines, out, False), (_take_simple_outlines, simple, False),
                           (_take_outlines, plain, False))

    def clean_outlines_emit_dev(self, d_sxy, d_sz, d_right, d_flag):
        """The kept vertices of the last clean_outlines_dev on this context into device buffers (ints) of exactly its
        sizes, as simplified_outlines_emit_dev."""
        self._check(self._L.bs_clean_outlines_emit_dev(self._h, d_sxy or None, d_sz or None, d_right or None, d_flag or None))

    # ---- outline triangles: the clean rings of every label, holes included, as triangles (bs_outline_triangles) ----------
    def outline_triangles(self, label, top=None, n_labels=None, num=0, den=1, cell_log2=0):
        """Every label's clean rings as triangles over the clean vertices (include/bs_api.h, "outline triangles").
        Returns (OutlineTriangles, the CleanOutlines with their vertices, the SimpleOutlines without vertices, the plain
        Outlines without vertices)."""
        label, top, h, w, nl = _label_top("outline_triangles", label, top, n_labels)
        out, clean, simple, plain = _lib.OutlineTriangles(), _lib.CleanOutlines(), _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_outline_triangles(self._h, label.ctypes.data, _ptr(top), w, h, nl, int(num), int(den),
                                                 int(cell_log2), C.byref(out), C.byref(clean), C.byref(simple),
                                                 C.byref(plain)))
        return _take_chain(self._L, (_take_outline_triangles, out, True), (_take_clean_outlines, clean, True),
                           (_take_simple_outlines, simple, False), (_take_outlines, plain, False))

    def outline_triangles_dev(self, d_label, d_top, width, height, n_labels, num=0, den=1, cell_log2=0):
        """Device-resident count (bs_outline_triangles_count_dev): d_label and d_top (0: no Z) are device pointers (ints).
        Returns (OutlineTriangles with tri None, CleanOutlines with the vertex arrays None, SimpleOutlines, Outlines)."""
        out, clean, simple, plain = _lib.OutlineTriangles(), _lib.CleanOutlines(), _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_outline_triangles_count_dev(self._h, d_label or None, d_top or None, width, height,
                                                           int(n_labels), int(num), int(den), int(cell_log2), C.byref(out),
                                                           C.byref(clean), C.byref(simple), C.byref(plain)))
        return _take_chain(self._L, (_take_outline_triangles, out, False), (_take_clean_outlines, clean, False),
                           (_take_simple_outlines, simple, False), (_take_outlines, plain, False))

    def outline_triangles_emit_dev(self, d_tri):
        """The triangles of the last outline_triangles_dev on this context into a device buffer (int) of
        [n_triangles][3] int32."""
        self._check(self._L.bs_outline_triangles_emit_dev(self._h, d_tri or None))

    def roof_mesh(self, roof_facets, solids, tolerance_mm=0, bin=None, sweeps=None):
        """outline_triangles() of the facet image of roof_facets() / roof_structure() with the tops of solids(), at a
        tolerance in millimetres (bin: the pixel edge, by default the Solids'), beside roof_polygons(clean=True): returns
        (OutlineTriangles, CleanOutlines, the plain Outlines).  sweeps: the sweep mode of the call (set_outline_sweeps)."""
        _facet_and_top("roof_mesh", roof_facets, solids, "outline_triangles_dev")
        num, den = simplify_tolerance(tolerance_mm, solids.bin if bin is None else bin)
        with self._sweeps(sweeps), self._bases(getattr(solids, "base", None)):
            t, c, _, plain = self.outline_triangles(roof_facets.facet, solids.top, n_labels=roof_facets.n_facets, num=num,
                                                    den=den)
        return t, c, plain

    # ---- polygon solids: a closed mesh per building over the clean vertices and the triangles (bs_poly_solids) ------------
    def poly_solids(self, label, top, label_building, n_labels=None, n_buildings=None, num=0, den=1, bin=1, base_z=0,
                    cell_log2=0):
        """Roof, floor and walls of every building as one closed mesh over the clean vertices (include/bs_api.h, "polygon
        solids").  label is [height][width], top [height][width][4] as Solids.top, label_building [n_labels] the building
        of every label.  n_labels defaults to label.max() + 1, n_buildings to label_building.max() + 1.  Returns
        (PolySolids, OutlineTriangles, the CleanOutlines with their vertices, the SimpleOutlines without vertices, the
        plain Outlines without vertices)."""
        label, top, h, w, nl = _label_top("poly_solids", label, top, n_labels, need_top=True)
        lb = np.ascontiguousarray(label_building, dtype=np.int32).reshape(-1)
        if len(lb) != nl:
            raise ValueError("poly_solids: label_building must have one entry per label")
        nb = (int(lb.max()) + 1 if nl else 0) if n_buildings is None else int(n_buildings)
        out, tri, clean = _lib.PolySolids(), _lib.OutlineTriangles(), _lib.CleanOutlines()
        simple, plain = _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_poly_solids(self._h, label.ctypes.data, top.ctypes.data, w, h, nl, int(num), int(den),
                                           int(cell_log2), lb.ctypes.data if nl else None, nb, int(bin), int(base_z),
                                           C.byref(out), C.byref(tri), C.byref(clean), C.byref(simple), C.byref(plain)))
        return _take_chain(self._L, (_take_poly_solids, out, True), (_take_outline_triangles, tri, True),
                           (_take_clean_outlines, clean, True), (_take_simple_outlines, simple, False),
                           (_take_outlines, plain, False))

    def poly_solids_dev(self, d_label, d_top, width, height, n_labels, d_label_building, n_buildings, num=0, den=1, bin=1,
                        base_z=0, cell_log2=0):
        """Device-resident count (bs_poly_solids_count_dev): d_label, d_top and d_label_building are device pointers
        (ints).  Returns (PolySolids with the mesh None and the sizes n_vertices / n_faces / n_indices of the buffers
        poly_solids_emit_dev fills, OutlineTriangles, CleanOutlines, SimpleOutlines, Outlines, all without their arrays
        of the emits)."""
        out, tri, clean = _lib.PolySolids(), _lib.OutlineTriangles(), _lib.CleanOutlines()
        simple, plain = _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_poly_solids_count_dev(self._h, d_label or None, d_top or None, width, height, int(n_labels),
                                                     int(num), int(den), int(cell_log2), d_label_building or None,
                                                     int(n_buildings), int(bin), int(base_z), C.byref(out), C.byref(tri),
                                                     C.byref(clean), C.byref(simple), C.byref(plain)))
        return _take_chain(self._L, (_take_poly_solids, out, False), (_take_outline_triangles, tri, False),
                           (_take_clean_outlines, clean, False), (_take_simple_outlines, simple, False),
                           (_take_outlines, plain, False))

    def poly_solids_emit_dev(self, d_vertex, d_face_offset, d_face_index, d_face_building, d_face_kind):
        """The mesh of the last poly_solids_dev on this context into device buffers (ints) of exactly its sizes."""
        self._check(self._L.bs_poly_solids_emit_dev(self._h, d_vertex or None, d_face_offset or None, d_face_index or None,
                                                    d_face_building or None, d_face_kind or None))

    def building_model(self, roof_facets, solids, tolerance_mm=0, bin=None, sweeps=None):
        """poly_solids() of the facet image and facet_building of roof_facets() / roof_structure() with the tops, bin and
        base_z of solids(), at a tolerance in millimetres, beside roof_mesh(): returns (PolySolids, OutlineTriangles,
        CleanOutlines, the plain Outlines).  sweeps: the sweep mode of the call (set_outline_sweeps)."""
        _facet_and_top("building_model", roof_facets, solids, "poly_solids_dev")
        b = solids.bin if bin is None else bin
        num, den = simplify_tolerance(tolerance_mm, b)
        with self._sweeps(sweeps), self._bases(getattr(solids, "base", None)):
            p, t, c, _, plain = self.poly_solids(roof_facets.facet, solids.top, roof_facets.facet_building,
                                                 n_labels=roof_facets.n_facets, n_buildings=solids.n_buildings, num=num,
                                                 den=den, bin=b, base_z=solids.base_z)
        return p, t, c, plain

    # ---- model raster: the outline triangles back on the lattice, and the model's error (bs_model_raster) -----------------
    def model_raster(self, label, top, n_labels=None, num=0, den=1, cell_log2=0, images=True):
        """The outline triangles of the images rasterised back onto the pixel lattice (include/bs_api.h, "model raster").
        label is [height][width], top [height][width][4] as Solids.top.  images=False leaves the three images out (None)
        and computes the figures alone.  Returns (ModelRaster, OutlineTriangles, the CleanOutlines with their vertices, the
        SimpleOutlines without vertices, the plain Outlines without vertices)."""
        label, top, h, w, nl = _label_top("model_raster", label, top, n_labels, need_top=True)
        img = [np.empty((h, w), np.int32) for _ in range(3)] if images else [None] * 3
        out, tri, clean = _lib.ModelRaster(), _lib.OutlineTriangles(), _lib.CleanOutlines()
        simple, plain = _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_model_raster(self._h, label.ctypes.data, top.ctypes.data, w, h, nl, int(num), int(den),
                                            int(cell_log2), *[_ptr(a) for a in img],
                                            C.byref(out), C.byref(tri), C.byref(clean), C.byref(simple), C.byref(plain)))
        return _take_chain(self._L, (_take_model_raster, out, *img), (_take_outline_triangles, tri, True),
                           (_take_clean_outlines, clean, True), (_take_simple_outlines, simple, False),
                           (_take_outlines, plain, False))

    def model_raster_dev(self, d_label, d_top, width, height, d_model=0, d_cover=0, d_mz2=0):
        """Device-resident raster (bs_model_raster_dev) of the triangles that the last outline_triangles_dev or
        poly_solids_dev left on this context, which it does not change: d_label and d_top are device pointers (ints) to
        images of the size of that count; d_model, d_cover, d_mz2 device pointers to int32 [height][width] or 0.  Returns
        the ModelRaster with its images None."""
        out = _lib.ModelRaster()
        self._check(self._L.bs_model_raster_dev(self._h, d_label or None, d_top or None, int(width), int(height),
                                                d_model or None, d_cover or None, d_mz2 or None, C.byref(out)))
        return _take_model_raster(self._L, out)

    def model_fidelity(self, roof_facets, solids, tolerance_mm=0, bin=None, sweeps=None):
        """What the polygon model of building_model() at this tolerance costs, per building: model_raster() of the facet
        image of roof_facets() / roof_structure() with the tops of solids(), its per-label figures added up by
        facet_building.  sweeps: the sweep mode of the call (set_outline_sweeps).  Returns (ModelFidelity,
        ModelRaster)."""
        _facet_and_top("model_fidelity", roof_facets, solids, "model_raster_dev")
        num, den = simplify_tolerance(tolerance_mm, solids.bin if bin is None else bin)
        with self._sweeps(sweeps), self._bases(getattr(solids, "base", None)):
            r = self.model_raster(roof_facets.facet, solids.top, n_labels=roof_facets.n_facets, num=num, den=den)[0]
        return model_fidelity_of(r, roof_facets.facet_building, solids.n_buildings), r

    # ---- point residuals: every point of the cloud against the polygon model (bs_point_residuals) -------------------------
    def point_residuals(self, label, top, xyz, n_labels=None, num=0, den=1, cell_log2=0, bin=1, plane_idx=None,
                        label_plane=None, clip2=None, outputs=True):
        """Every point of the cloud against the outline triangles of the images (include/bs_api.h, "point residuals").
        label is [height][width], top [height][width][4] as Solids.top, xyz [n][3] int32 millimetres shifted to the origin
        of the images.  plane_idx [n] and label_plane [n_labels] come together or not at all.  clip2: the inlier bound in
        doubled millimetres, None for no clipping.  outputs=False leaves the three per-point arrays out (None) and computes
        the figures alone.  Returns (PointResiduals, OutlineTriangles, the CleanOutlines with their vertices, the
        SimpleOutlines without vertices, the plain Outlines without vertices)."""
        label, top, h, w, nl = _label_top("point_residuals", label, top, n_labels, need_top=True)
        xyz = _points("point_residuals", xyz)
        n = len(xyz)
        pi, lp = _plane_pair("point_residuals", plane_idx, label_plane, n, nl)
        arr = [np.empty(n, np.int32) for _ in range(3)] if outputs else [None] * 3
        out, tri, clean = _lib.PointResiduals(), _lib.OutlineTriangles(), _lib.CleanOutlines()
        simple, plain = _lib.SimpleOutlines(), _lib.Outlines()
        self._check(self._L.bs_point_residuals(self._h, label.ctypes.data, top.ctypes.data, w, h, nl, int(num), int(den),
                                               int(cell_log2), xyz.ctypes.data, n, int(bin), _ptr(pi), _ptr(lp),
                                               _clip2(clip2), *[_ptr(a) for a in arr], C.byref(out), C.byref(tri),
                                               C.byref(clean), C.byref(simple), C.byref(plain)))
        return _take_chain(self._L, (_take_point_residuals, out, *arr), (_take_outline_triangles, tri, True),
                           (_take_clean_outlines, clean, True), (_take_simple_outlines, simple, False),
                           (_take_outlines, plain, False))

    def point_residuals_dev(self, d_xyz, n, bin=1, d_plane_idx=0, label_plane=None, clip2=None, d_label_out=0, d_r2=0,
                            d_cover=0):
        """Device-resident stage (bs_point_residuals_dev) over the triangles that the last outline_triangles_dev or
        poly_solids_dev left on this context, which it does not change: d_xyz [n][3] and d_plane_idx [n] are device pointers
        (ints), label_plane a host table of that count's n_labels; d_label_out, d_r2, d_cover device pointers to int32 [n]
        or 0.  Returns the PointResiduals with its per-point arrays None."""
        lp = None if label_plane is None else np.ascontiguousarray(label_plane, dtype=np.int32).reshape(-1)
        out = _lib.PointResiduals()
        self._check(self._L.bs_point_residuals_dev(self._h, d_xyz or None, int(n), int(bin), d_plane_idx or None,
                                                   _ptr(lp), _clip2(clip2),
                                                   d_label_out or None, d_r2 or None, d_cover or None, C.byref(out)))
        if lp is not None and len(lp) != out.n_labels:
            _free(self._L, out)
            raise ValueError("point_residuals_dev: label_plane must have one entry per label of the count")
        return _take_point_residuals(self._L, out)

    def point_fidelity(self, xyz, roof_facets, solids, tolerance_mm=0, plane_idx=None, clip_mm=None, bin=None, sweeps=None):
        """How far the polygon model of building_model() at this tolerance lies from the points it was built from, per
        building, beside model_fidelity(): point_residuals() of the cloud against the facet image of roof_facets() /
        roof_structure() with the tops of solids(), its per-label figures added up by facet_building.  plane_idx: the
        planes of the points, compared with facet_plane.  clip_mm: the inlier bound in millimetres, None for no clipping.
        sweeps: the sweep mode of the call (set_outline_sweeps).  Returns (PointFidelity, PointResiduals)."""
        _facet_and_top("point_fidelity", roof_facets, solids, "point_residuals_dev")
        b = solids.bin if bin is None else bin
        num, den = simplify_tolerance(tolerance_mm, b)
        if clip_mm is not None and (int(clip_mm) != clip_mm or clip_mm < 0):
            raise ValueError("point_fidelity: clip_mm must be a whole number >= 0")
        with self._sweeps(sweeps), self._bases(getattr(solids, "base", None)):
            r = self.point_residuals(roof_facets.facet, solids.top, xyz, n_labels=roof_facets.n_facets, num=num, den=den, bin=b,
                                     plane_idx=plane_idx, label_plane=None if plane_idx is None else roof_facets.facet_plane,
                                     clip2=None if clip_mm is None else 2 * int(clip_mm), outputs=False)[0]
        return point_fidelity_of(r, roof_facets.facet_building, solids.n_buildings), r

    # ---- per-building bases: solids that stand on the terrain (bs_set_building_bases, include/bs_api.h) --------------------
    def set_building_bases(self, base):
        """The base of every building for solids(), generalise_roofs() and poly_solids() on this context, in place of
        their scalar base_z (bs_set_building_bases): base [n_buildings] int32, in the pipeline Terrain.ground.  None
        switches it off, the default.  A call over another number of buildings is refused while it is set."""
        if base is None:
            self._check(self._L.bs_set_building_bases(self._h, None, 0))
            return
        b = np.ascontiguousarray(base, dtype=np.int32).reshape(-1)
        if not np.array_equal(b, np.asarray(base).reshape(-1)):
            raise ValueError("set_building_bases: the bases must be whole numbers that fit 32 bits")
        self._check(self._L.bs_set_building_bases(self._h, b.ctypes.data if len(b) else None, len(b)))

    def building_bases(self):
        """The table of set_building_bases() as the context holds it (bs_get_building_bases), or None while it is off."""
        n = C.c_int32(0)
        self._check(self._L.bs_get_building_bases(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        b = np.empty(n.value, np.int32)
        self._check(self._L.bs_get_building_bases(self._h, b.ctypes.data, n.value, C.byref(n)))
        return b

    @contextmanager
    def _bases(self, base):
        """the building bases for one call (None: off), the previous table restored behind it"""
        prev = self.building_bases()
        self.set_building_bases(base)
        try:
            yield
        finally:
            self.set_building_bases(prev)

    # ---- terrain: the ground height of every building from the points around it (bs_terrain, include/bs_api.h) ----------
    def terrain(self, xyz, bmap, buildings_or_n, bin=100, ring=10, q=(1, 2), min_ground=8, fallback_z=0, images=True):
        """The ground every building stands on, read from the lowest points of the pixels just outside its footprint
        (include/bs_api.h, "terrain").  xyz [n][3] int32 millimetres shifted to its origin, bmap the building map,
        buildings_or_n the Buildings of building_map() or their number.  ring: how many pixels the ring reaches out;
        q = (num, den): the quantile of the ring pixels' lowest points that becomes `ground`; min_ground: the fewest ring
        pixels with a point that a quantile is taken of; fallback_z: the ground of a building with fewer.  images=False leaves
        the three images out (None).  Returns Terrain."""
        xyz = _points("terrain", xyz)
        bmap = np.ascontiguousarray(bmap, dtype=np.int32)
        if bmap.ndim != 2 or bmap.size == 0:
            raise ValueError("terrain: bmap must be [height][width]")
        h, w = bmap.shape
        nb = int(getattr(buildings_or_n, "n_buildings", buildings_or_n))
        owner, dist, low = ((np.empty((h, w), np.int32), np.empty((h, w), np.uint8), np.empty((h, w), np.int32)) if images
                            else (None, None, None))
        out = _lib.Terrain()
        self._check(self._L.bs_terrain(self._h, xyz.ctypes.data, len(xyz), int(bin), bmap.ctypes.data, w, h, nb, int(ring),
                                       *_quantile(q), int(min_ground), int(fallback_z),
                                       *[_ptr(a) for a in (owner, dist, low)], C.byref(out)))
        return _take_terrain(self._L, out, owner, dist, low)

    def terrain_dev(self, d_xyz, n, d_map, width, height, n_buildings, bin=100, ring=10, q=(1, 2), min_ground=8, fallback_z=0,
                    d_owner=0, d_dist=0, d_low=0):
        """Device-resident stage (bs_terrain_dev): d_xyz [n][3] int32 and d_map [height][width] int32 are device pointers
        (ints); d_owner (int32), d_dist (uint8) and d_low (int32), [height][width] each, are device pointers or 0.  Returns
        the Terrain with its images None."""
        out = _lib.Terrain()
        self._check(self._L.bs_terrain_dev(self._h, d_xyz or None, int(n), int(bin), d_map or None, int(width), int(height),
                                           int(n_buildings), int(ring), *_quantile(q), int(min_ground), int(fallback_z),
                                           d_owner or None, d_dist or None, d_low or None, C.byref(out)))
        return _take_terrain(self._L, out)

    # ---- ground: a terrain raster of the tile by a progressive morphological filter (bs_ground, include/bs_api.h) ---------
    def ground(self, xyz, extent=None, params=None, images=True, points=True, **kw):
        """The ground surface of a cloud shifted to its origin, per pixel of a lattice of params["cell"] millimetres
        (include/bs_api.h, "ground").  params: a dict of ground_params(), or its keywords directly.  images=False leaves
        low, dtm and step out (None), points=False hag and cls.  Returns Ground."""
        xyz = _points("ground", xyz)
        p = ground_params(**kw) if params is None else dict(params, **kw)
        ext = np.ascontiguousarray(xyz.max(0) if extent is None else extent, dtype=np.int32)
        w, h = grid_dims(ext, p["cell"])
        low, dtm, step = ((np.empty((h, w), np.int32), np.empty((h, w), np.int32), np.empty((h, w), np.uint8)) if images
                          else (None, None, None))
        hag, cls = (np.empty(len(xyz), np.int32), np.empty(len(xyz), np.uint8)) if points else (None, None)
        out = _lib.Ground()
        self._check(self._L.bs_ground(self._h, xyz.ctypes.data, len(xyz), ext.ctypes.data, C.byref(_ground_struct(p)),
                                      *[_ptr(a) for a in (low, dtm, step, hag, cls)],
                                      C.byref(out)))
        return _take_ground(self._L, out, p, low, dtm, step, hag, cls)

    def ground_dev(self, d_xyz, n, extent, params=None, d_low=0, d_dtm=0, d_step=0, d_hag=0, d_class=0, **kw):
        """Device-resident stage (bs_ground_dev): d_xyz [n][3] int32 is a device pointer (int); d_low, d_dtm (int32
        [height][width]), d_step (uint8 [height][width]), d_hag (int32 [n]) and d_class (uint8 [n]) are device pointers or
        0.  Returns the Ground with its arrays None."""
        p = ground_params(**kw) if params is None else dict(params, **kw)
        ext = np.ascontiguousarray(extent, dtype=np.int32)
        out = _lib.Ground()
        self._check(self._L.bs_ground_dev(self._h, d_xyz or None, int(n), ext.ctypes.data, C.byref(_ground_struct(p)),
                                          d_low or None, d_dtm or None, d_step or None, d_hag or None, d_class or None,
                                          C.byref(out)))
        return _take_ground(self._L, out, p)

    def set_ground_model(self, dtm, cell=None, min_height=None, device=False):
        """The ground surface that grid_picture(), assign_buildings() and roofs() on this context measure "above ground"
        against, in place of their scalar ground_th (bs_set_ground_model): dtm [height][width] int32 over a lattice of
        `cell` millimetres, INT32_MAX where it holds nothing; a point counts iff z >= dtm[pixel] + min_height.  dtm may be a
        Ground (its dtm, cell and min_height are the defaults).  None switches it off, the default.  device=True: dtm is
        (device pointer, width, height)."""
        if dtm is None:
            self._check(self._L.bs_set_ground_model(self._h, None, 0, 0, 0, 0))
            return
        if isinstance(dtm, Ground):
            cell = dtm.cell if cell is None else cell
            min_height = dtm.min_height if min_height is None else min_height
            dtm = dtm.dtm
        if cell is None or min_height is None:
            raise ValueError("set_ground_model: cell and min_height are needed")
        if device:
            ptr, w, h = dtm
            self._check(self._L.bs_set_ground_model_dev(self._h, ptr or None, int(w), int(h), int(cell), int(min_height)))
            return
        if dtm is None:
            raise ValueError("set_ground_model: this Ground holds no dtm (images=False, or ground_dev)")
        t = np.ascontiguousarray(dtm, dtype=np.int32)
        if t.ndim != 2 or t.size == 0 or not np.array_equal(t, np.asarray(dtm)):
            raise ValueError("set_ground_model: dtm must be [height][width] whole numbers that fit 32 bits")
        self._check(self._L.bs_set_ground_model(self._h, t.ctypes.data, t.shape[1], t.shape[0], int(cell), int(min_height)))

    def ground_model(self):
        """(dtm [height][width] int32, cell, min_height) as the context holds it (bs_get_ground_model), or None while the
        switch is off."""
        w, h, cell, mh = (C.c_int32(0) for _ in range(4))
        self._check(self._L.bs_get_ground_model(self._h, None, 0, C.byref(w), C.byref(h), C.byref(cell), C.byref(mh)))
        if w.value == 0:
            return None
        t = np.empty((h.value, w.value), np.int32)
        self._check(self._L.bs_get_ground_model(self._h, t.ctypes.data, t.size, C.byref(w), C.byref(h), C.byref(cell),
                                                C.byref(mh)))
        return t, cell.value, mh.value

    @contextmanager
    def _ground_model(self, ground):
        """the ground model for one call (None: off), the previous one restored behind it"""
        prev = self.ground_model()
        self.set_ground_model(ground)
        try:
            yield
        finally:
            if prev is None:
                self.set_ground_model(None)
            else:
                self.set_ground_model(prev[0], prev[1], prev[2])

    # ---- roof evidence and the footprint screen (bs_roof_evidence, bs_set_footprint_screen; include/bs_api.h) ------------------
    def roof_evidence(self, xyz, plane_idx, n_planes, plane_ok=None, extent=None, bin=100, ground_th=0.0, params=None, images=True,
                      **kw):
        """Per pixel of the raster's lattice, whether the points above ground look like a roof (include/bs_api.h, "roof
        evidence"): the share of them on a plane that counts (plane_ok uint8 [n_planes] of plane_quality(); None: every plane),
        over a (2r+1)^2 window.  ground_th is the raster's; a ground model of the context takes its place.  params: a dict of
        evidence_params(), or its keywords directly.  images=False leaves everything but keep out.  Returns RoofEvidence."""
        xyz = _points("roof_evidence", xyz)
        pi = _point_labels("roof_evidence", "plane_idx", plane_idx, xyz)
        p = evidence_params(**kw) if params is None else dict(params, **kw)
        ok = _plane_ok(plane_ok, n_planes)
        ext = np.ascontiguousarray(xyz.max(0) if extent is None else extent, dtype=np.int32)
        w, h = grid_dims(ext, bin)
        keep = np.empty((h, w), np.uint8)
        imgs = [np.empty((h, w), np.int32) if images else None for _ in range(4)]
        out = _lib.RoofEvidence()
        self._check(self._L.bs_roof_evidence(self._h, xyz.ctypes.data, len(xyz), pi.ctypes.data, int(n_planes),
                                             _ptr(ok) if int(n_planes) else None, ext.ctypes.data, int(bin),
                                             float(ground_th), p["r"], p["min_points"], p["num"], p["den"], keep.ctypes.data,
                                             *[_ptr(a) for a in imgs], C.byref(out)))
        return _take_evidence(out, n_planes, ok, keep, *imgs)

    def roof_evidence_dev(self, d_xyz, n, d_plane_idx, n_planes, extent, d_keep, plane_ok=None, bin=100, ground_th=0.0,
                          params=None, d_above=0, d_planar=0, d_win_above=0, d_win_planar=0, **kw):
        """Device-resident stage (bs_roof_evidence_dev): d_xyz [n][3] and d_plane_idx [n] int32, d_keep (uint8
        [height][width]) and the optional int32 images are device pointers (ints); plane_ok stays a host table.  Returns the
        RoofEvidence with its images None."""
        p = evidence_params(**kw) if params is None else dict(params, **kw)
        ok = _plane_ok(plane_ok, n_planes)
        ext = np.ascontiguousarray(extent, dtype=np.int32)
        out = _lib.RoofEvidence()
        self._check(self._L.bs_roof_evidence_dev(self._h, d_xyz or None, int(n), d_plane_idx or None, int(n_planes),
                                                 _ptr(ok) if int(n_planes) else None, ext.ctypes.data,
                                                 int(bin), float(ground_th), p["r"], p["min_points"], p["num"], p["den"],
                                                 d_keep or None, d_above or None, d_planar or None, d_win_above or None,
                                                 d_win_planar or None, C.byref(out)))
        return _take_evidence(out, n_planes, ok)

    def set_footprint_screen(self, keep, device=False):
        """The image that footprints() on this context ANDs into its thresholded mask before the closing
        (bs_set_footprint_screen): keep [height][width], non-zero = the pixel may be foreground; a RoofEvidence stands for its
        keep.  None switches it off, the default.  device=True: keep is (device pointer, width, height); the image is not
        copied and must outlive the switch."""
        self._screen_dev = None
        if keep is None:
            self._check(self._L.bs_set_footprint_screen(self._h, None, 0, 0))
            return
        if device:
            ptr, w, h = keep
            self._check(self._L.bs_set_footprint_screen_dev(self._h, ptr or None, int(w), int(h)))
            self._screen_dev = (ptr, int(w), int(h)) if ptr else None
            return
        if isinstance(keep, RoofEvidence):
            keep = keep.keep
            if keep is None:
                raise ValueError("set_footprint_screen: this RoofEvidence holds no keep image (roof_evidence_dev)")
        k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if k.ndim != 2 or k.size == 0:
            raise ValueError("set_footprint_screen: keep must be [height][width]")
        self._check(self._L.bs_set_footprint_screen(self._h, k.ctypes.data, k.shape[1], k.shape[0]))

    def footprint_screen(self):
        """keep uint8 [height][width] as the context reads it now (bs_get_footprint_screen), or None while the switch is off."""
        w, h = C.c_int32(0), C.c_int32(0)
        self._check(self._L.bs_get_footprint_screen(self._h, None, 0, C.byref(w), C.byref(h)))
        if w.value == 0:
            return None
        k = np.empty((h.value, w.value), np.uint8)
        self._check(self._L.bs_get_footprint_screen(self._h, k.ctypes.data, k.size, C.byref(w), C.byref(h)))
        return k

    @contextmanager
    def _footprint_screen(self, keep):
        """the footprint screen for one call, the previous one (a device image as the pointer it was) restored behind it"""
        prev_dev = getattr(self, "_screen_dev", None)
        prev = None if prev_dev else self.footprint_screen()
        self.set_footprint_screen(keep)
        try:
            yield
        finally:
            if prev_dev:
                self.set_footprint_screen(prev_dev, device=True)
            else:
                self.set_footprint_screen(prev)

    def _evidence(self, xyz, plane_idx, n_planes, bin, ground_th, evidence):
        """plane_fit -> plane_quality -> roof_evidence for evidence= of buildings()"""
        p = evidence_params(**evidence)
        fit = self.plane_fit(xyz, plane_idx, n_planes)
        ok = plane_quality(fit, p["min_plane_points"], p["max_rms_mm"])
        ev = self.roof_evidence(xyz, plane_idx, n_planes, ok, bin=bin, ground_th=ground_th, params=p, images=False)
        ev.fit = fit
        if ev.n_planes > 0 and ev.planes_ok == 0:
            warnings.warn(f"evidence: none of the {ev.n_planes} planes passes the quality rule (max_rms_mm={p['max_rms_mm']}, "
                          f"min_plane_points={p['min_plane_points']}): the screen rejects every pixel and no building will be found; "
                          "read RoofEvidence.fit (r_sq_sum / n_points) and choose max_rms_mm from it", RuntimeWarning, stacklevel=3)
        return ev


def evidence_params(r=3, min_points=1, share=(1, 2), min_plane_points=0, max_rms_mm=100):
    """The parameters of Context.roof_evidence() and of evidence= as a dict: r (pixels, the window is (2r+1)^2), min_points
    (counting points a window needs), num / den (the share of them that must lie on a good plane), and the rule of
    plane_quality() that says which planes are good: min_plane_points and max_rms_mm."""
    return dict(r=int(r), min_points=int(min_points), num=int(share[0]), den=int(share[1]),
                min_plane_points=int(min_plane_points), max_rms_mm=int(max_rms_mm))


def plane_quality(fits, min_points=0, max_rms_mm=100) -> np.ndarray:
    """ok uint8 [n_planes] of a PlaneFits (bs_plane_quality; host only): a plane counts iff it was fitted, has at least
    min_points points and the rms residual of its fit is at most max_rms_mm -- exactly, in integers: r_sq_sum <= max_rms_mm^2
    * n_points.  The slabs the grower cuts out of a tree crown fail it."""
    L = _lib.load()
    n = int(fits.n_planes)
    arrs = {k: np.ascontiguousarray(getattr(fits, k), dtype=dt).reshape(-1)
            for k, dt in (("status", np.int32), ("n_points", np.int64), ("r_sq_sum", np.int64))}
    if any(len(a) != n for a in arrs.values()):
        raise ValueError("plane_quality: status, n_points and r_sq_sum must be [n_planes]")
    f = _lib.PlaneFits()
    f.n_planes = n
    f.status = arrs["status"].ctypes.data_as(C.POINTER(C.c_int32))
    f.n_points = arrs["n_points"].ctypes.data_as(C.POINTER(C.c_int64))
    f.r_sq_sum = arrs["r_sq_sum"].ctypes.data_as(C.POINTER(C.c_int64))
    ok = np.zeros(n, np.uint8)
    rc = L.bs_plane_quality(C.byref(f), int(min_points), int(max_rms_mm), ok.ctypes.data if n else None)
    if rc != _lib.BS_OK:
        raise BsError(rc, "plane quality: min_points < 0 or max_rms_mm outside 0 .. 32767")
    return ok


@dataclass
class RoofEvidence:
    """bs_roof_evidence: the lattice, the parameters of the call, the figures, and the images [height][width]: keep (uint8, what
    Context.set_footprint_screen() takes), above, planar, win_above, win_planar (int32).  plane_ok is the table the call
    counted by (None: every plane), n_planes its length and planes_ok how many of its planes count: with planes_ok == 0 <
    n_planes nothing is planar and keep is all zero.  The images are None after roof_evidence_dev or where they were switched
    off."""
    width: int
    height: int
    r: int
    min_points: int
    num: int
    den: int
    grid: int
    tile: int
    max_window: int
    n_points: int
    n_counted: int
    n_planar: int
    n_pixels: int
    pixels_kept: int
    pixels_rejected: int
    pixels_thin: int
    n_planes: int = 0
    planes_ok: int = 0
    info: dict = field(default_factory=dict)
    plane_ok: np.ndarray | None = field(default=None, repr=False)
    keep: np.ndarray | None = field(default=None, repr=False)
    above: np.ndarray | None = field(default=None, repr=False)
    planar: np.ndarray | None = field(default=None, repr=False)
    win_above: np.ndarray | None = field(default=None, repr=False)
    win_planar: np.ndarray | None = field(default=None, repr=False)
    fit: PlaneFits | None = field(default=None, repr=False)  # the fit plane_ok was judged by, after evidence=


def _take_evidence(out, n_planes, plane_ok=None, keep=None, above=None, planar=None, win_above=None, win_planar=None) -> RoofEvidence:
    head = {n: getattr(out, n) for n in _lib.EVIDENCE_NARROW[:-1] + _lib.EVIDENCE_WIDE}
    head.update(n_planes=int(n_planes), planes_ok=int(n_planes) if plane_ok is None else int(np.count_nonzero(plane_ok)))
    return RoofEvidence(**head, info={n: getattr(out, n) for n in _lib.EVIDENCE_MS}, plane_ok=plane_ok, keep=keep, above=above,
                        planar=planar, win_above=win_above, win_planar=win_planar)


def _plane_ok(plane_ok, n_planes):
    if plane_ok is None:
        return None
    ok = np.ascontiguousarray(np.asarray(plane_ok) != 0, dtype=np.uint8).reshape(-1)
    if len(ok) != int(n_planes):
        raise ValueError("roof_evidence: plane_ok must be [n_planes]")
    return ok


def ground_params(cell=500, max_radius_mm=12800, slope=(3, 10), dh0=200, dh_max=2500, tol=200, min_height=2000, radius=None):
    """The parameters of Context.ground() as a dict: cell (mm), radius (pixels per step; by default doubled 1, 2, 4, ...
    while r * cell <= max_radius_mm), s_num / s_den (the slope), dh0, dh_max, tol, min_height (mm)."""
    if radius is None:
        radius, r = [], 1
        while r * cell <= max_radius_mm and r <= _lib.GROUND_MAX_RADIUS and len(radius) < _lib.GROUND_MAX_STEPS:
            radius.append(r)
            r *= 2
    return dict(cell=int(cell), radius=[int(r) for r in radius], s_num=int(slope[0]), s_den=int(slope[1]), dh0=int(dh0),
                dh_max=int(dh_max), tol=int(tol), min_height=int(min_height))


def _ground_struct(p):
    q = _lib.GroundParams()
    rad = list(p["radius"])
    if len(rad) > _lib.GROUND_MAX_STEPS:
        raise ValueError("ground: more than 16 steps")
    q.cell, q.n_steps = int(p["cell"]), len(rad)
    for k, r in enumerate(rad):
        q.radius[k] = int(r)
    for k in ("s_num", "s_den", "dh0", "dh_max", "tol", "min_height"):
        setattr(q, k, int(p[k]))
    return q


@dataclass
class Ground:
    """bs_ground: the lattice (width, height, cell), the steps (radius, threshold, step_pixels: lists of n_steps), the
    figures, and the arrays: low (the lowest point of every pixel, INT32_MAX: none), dtm (the ground surface, INT32_MAX:
    nothing within reach), step (0: ground, k: removed in step k, 255: no point), hag (every point's height above dtm)
    and cls (0 ground, 1 low, 2 object).  tol and min_height are the parameters of the call; a Ground is what
    Context.set_ground_model() takes.  The arrays are None after ground_dev or where they were switched off."""
    width: int
    height: int
    cell: int
    n_steps: int
    radius: list
    threshold: list
    step_pixels: list
    grid: int
    row_lds: int
    n_points: int
    n_ground_pixels: int
    n_object_pixels: int
    n_empty_pixels: int
    n_filled_pixels: int
    n_ground_points: int
    n_low_points: int
    n_object_points: int
    sum_hag_ground: int
    dtm_min: int
    dtm_max: int
    hag_min: int
    hag_max: int
    tol: int
    min_height: int
    info: dict = field(default_factory=dict)
    low: np.ndarray | None = field(default=None, repr=False)
    dtm: np.ndarray | None = field(default=None, repr=False)
    step: np.ndarray | None = field(default=None, repr=False)
    hag: np.ndarray | None = field(default=None, repr=False)
    cls: np.ndarray | None = field(default=None, repr=False)


def _take_ground(L, out, p, low=None, dtm=None, step=None, hag=None, cls=None) -> Ground:
    """Copy a bs_ground into Python values and release it."""
    try:
        k = out.n_steps
        head = {n: getattr(out, n) for n in _lib.GROUND_HEAD + _lib.GROUND_NARROW + _lib.GROUND_WIDE + ("n_points",)}
        lists = {n: list(getattr(out, n))[:k] for n in _lib.GROUND_TABLES + ("step_pixels",)}
        info = {n: getattr(out, n) for n in _lib.GROUND_MS}
        info["ms_step"] = list(out.ms_step)[:k]
        return Ground(**head, **lists, tol=int(p["tol"]), min_height=int(p["min_height"]), info=info, low=low, dtm=dtm,
                      step=step, hag=hag, cls=cls)
    finally:
        _free(L, out)


@dataclass
class Terrain:
    """bs_terrain: the parameters, the totals, the per-building figures (ring_pixels, ground_pixels, ring_points,
    ground_sum, ground_min, ground_max, ground, status: 0 the quantile, 1 fallback_z) and the three images: owner (the
    building whose ring reached the pixel, the building itself on its own pixels, -1: never reached), dist (the round that
    reached it) and low (the lowest point of a ring pixel, INT32_MAX: none, or no ring pixel).  `ground` is the table
    Context.set_building_bases() takes.  The images are None after terrain_dev or images=False."""
    width: int
    height: int
    n_buildings: int
    bin: int
    ring: int
    q_num: int
    q_den: int
    min_ground: int
    fallback_z: int
    fig_cap: int
    grid: int
    rounds_used: int
    n_fallback: int
    n_points: int
    n_ring_pixels: int
    n_ground_pixels: int
    n_ring_points: int
    ring_pixels: np.ndarray
    ground_pixels: np.ndarray
    ring_points: np.ndarray
    ground_sum: np.ndarray
    ground_min: np.ndarray
    ground_max: np.ndarray
    ground: np.ndarray
    status: np.ndarray
    info: dict = field(default_factory=dict)
    owner: np.ndarray | None = field(default=None, repr=False)
    dist: np.ndarray | None = field(default=None, repr=False)
    low: np.ndarray | None = field(default=None, repr=False)


def _quantile(q):
    num, den = q
    if int(num) != num or int(den) != den or not (0 <= num <= den and 1 <= den < 2 ** 31):
        raise ValueError("q must be (num, den), whole numbers with 0 <= num <= den and 1 <= den < 2^31")
    return int(num), int(den)


_TERRAIN_ARRAYS = _rows(_lib.TERRAIN_WIDE, np.int64) + _rows(_lib.TERRAIN_NARROW, np.int32)


def _take_terrain(L, out, owner=None, dist=None, low=None) -> Terrain:
    """Copy a bs_terrain into numpy arrays and release it."""
    n = out.n_buildings
    try:
        arrs = _copy_arrays(out, _TERRAIN_ARRAYS, n)
        head = {k: getattr(out, k) for k in _lib.TERRAIN_HEAD + _lib.TERRAIN_TOTALS if k != "reserved"}
        info = {k: getattr(out, k) for k in _lib.TERRAIN_MS}
        return Terrain(**head, **arrs, info=info, owner=owner, dist=dist, low=low)
    finally:
        _free(L, out)


@dataclass
class PlaneVotes:
    """Entry p - 1 is plane p: the building that holds most of its points (-1: none), that building's count, the
    plane's points, and those outside every building."""
    plane_building: np.ndarray
    votes_in: np.ndarray
    votes_total: np.ndarray
    votes_outside: np.ndarray


@dataclass
class Buildings:
    """bs_buildings: building c is contour c of the footprints of the same mask.  The pixel figures come from
    building_map, the point figures from assign_buildings."""
    n_buildings: int
    width: int
    height: int
    start_xy: np.ndarray
    bbox: np.ndarray
    pixels: np.ndarray
    fg_pixels: np.ndarray
    n_points: np.ndarray
    n_above: np.ndarray
    z_min: np.ndarray
    z_max: np.ndarray
    z_sum: np.ndarray
    info: dict = field(default_factory=dict)
    map: np.ndarray | None = field(default=None, repr=False)
    building_idx: np.ndarray | None = field(default=None, repr=False)
    ground_th: float = 0.0
    votes: PlaneVotes | None = None


_BUILDING_ARRAYS = (("start_xy", np.int32, 2), ("bbox", np.int32, 4), ("pixels", np.int64, 1), ("fg_pixels", np.int64, 1),
                    ("n_points", np.int64, 1), ("n_above", np.int64, 1), ("z_min", np.int32, 1), ("z_max", np.int32, 1),
                    ("z_sum", np.int64, 1))


def _take_buildings(L, out) -> Buildings:
    """Copy a bs_buildings into numpy arrays and release it."""
    n = out.n_buildings
    try:
        arrs = _copy_arrays(out, _BUILDING_ARRAYS, n)
        info = {k: getattr(out, k) for k in ("ms_label_mask", "ms_label_fill", "ms_number", "ms_map", "ms_assign")}
        return Buildings(n, out.width, out.height, info=info, **arrs)
    finally:
        _free(L, out)


def _buildings_struct(b: Buildings):
    """A bs_buildings whose arrays are b's own numpy arrays (the library reads and writes them in place)."""
    st = _lib.Buildings()
    st.n_buildings, st.width, st.height = b.n_buildings, b.width, b.height
    keep = []
    for name, dt, cols in _BUILDING_ARRAYS:
        a = getattr(b, name)
        if a.dtype != dt or not a.flags.c_contiguous or not a.flags.writeable or a.size != b.n_buildings * cols:
            raise ValueError(f"Buildings.{name} must be a contiguous {np.dtype(dt).name} array of {b.n_buildings * cols}")
        keep.append(a if a.size else np.zeros(cols, dt))  # (never a null pointer)
        setattr(st, name, keep[-1].ctypes.data_as(C.POINTER(C.c_int32 if dt == np.int32 else C.c_int64)))
    st._keep = keep
    return st


def write_buildings_obj(fp, buildings: Buildings, path, bin=100, origin=None, ground_th=None, min_area=500.0,
                        min_perimeter=100.0):
    """LoD1 OBJ in millimetres through the library's writer (bs_buildings_write_obj; the format is written down in
    include/bs_api.h): the kept footprints extruded from the ground threshold to the mean height of their
    above-ground points.  origin: the shift that was subtracted from the cloud; ground_th: default buildings.ground_th."""
    area = np.ascontiguousarray(fp.area, dtype=np.float64)
    per = np.ascontiguousarray(fp.perimeter, dtype=np.float64)
    if len(area) != len(fp.contours) or len(per) != len(fp.contours):
        raise ValueError("area and perimeter must have one entry per contour")
    c, keep = _contours_struct(fp)
    c.area = (area if area.size else _PAD).ctypes.data_as(C.POINTER(C.c_double))
    c.perimeter = (per if per.size else _PAD).ctypes.data_as(C.POINTER(C.c_double))
    st = _buildings_struct(buildings)
    th = buildings.ground_th if ground_th is None else ground_th
    _write_obj("bs_buildings_write_obj", path, "the contours and the buildings are not of the same mask", C.byref(c), C.byref(st),
               int(bin), _origin(origin), float(th), float(min_area), float(min_perimeter))


@dataclass
class Roofs:
    """bs_roofs: roof / support / height are the [height][width] int32 images (None where they stayed on the device
    or were not asked for); the per-plane arrays have entry p - 1 for plane p."""
    n_planes: int
    width: int
    image_height: int
    fill_rounds: int
    seeded_pixels: int
    filled_pixels: int
    unroofed_pixels: int
    pixels: np.ndarray
    seed_pixels: np.ndarray
    bbox: np.ndarray
    n_support: np.ndarray
    z_min: np.ndarray
    z_max: np.ndarray
    z_sum: np.ndarray
    info: dict = field(default_factory=dict)
    roof: np.ndarray | None = field(default=None, repr=False)
    support: np.ndarray | None = field(default=None, repr=False)
    height: np.ndarray | None = field(default=None, repr=False)
    home: np.ndarray | None = field(default=None, repr=False)
    normal: np.ndarray | None = field(default=None, repr=False)
    center: np.ndarray | None = field(default=None, repr=False)
    bin: int = 100
    fit: "PlaneFits | None" = field(default=None, repr=False)  # roof_model(refit=True)


_ROOF_ARRAYS = (("pixels", np.int64, 1), ("seed_pixels", np.int64, 1), ("bbox", np.int32, 4), ("n_support", np.int64, 1),
                ("z_min", np.int32, 1), ("z_max", np.int32, 1), ("z_sum", np.int64, 1))


def _roof_tables(home, normal, center):
    """(home int32 [n], normal f64 [n][3], center int32 [n][3]) as contiguous arrays that are never empty buffers"""
    home = np.ascontiguousarray(home, dtype=np.int32).reshape(-1)
    n = len(home)
    normal = np.ascontiguousarray(normal, dtype=np.float64).reshape(-1, 3)
    center = np.ascontiguousarray(center, dtype=np.int32).reshape(-1, 3)
    if len(normal) != n or len(center) != n:
        raise ValueError("home, normal and center must have one entry per plane")
    return home, normal, center


def _take_roofs(L, out, roof, support, height, tabs, bin) -> Roofs:
    """Copy a bs_roofs into numpy arrays and release it."""
    n = out.n_planes
    try:
        arrs = _copy_arrays(out, _ROOF_ARRAYS, n)
        info = {k: getattr(out, k) for k in ("ms_vote", "ms_fill", "ms_figures", "ms_height")}
        return Roofs(n, out.width, out.height, out.fill_rounds, out.seeded_pixels, out.filled_pixels,
                     out.unroofed_pixels, info=info, roof=roof, support=support, height=height, home=tabs[0],
                     normal=tabs[1], center=tabs[2], bin=bin, **arrs)
    finally:
        _free(L, out)


@dataclass
class PlaneFits:
    """bs_plane_fits: entry p - 1 is plane p.  status 0 = fitted, 1 = fewer than 3 points, 2 = too large for the exact
    sums; residual is the per-point image of plane_fit(residuals=True), else None."""
    n_planes: int
    status: np.ndarray
    n_points: np.ndarray
    center: np.ndarray
    normal: np.ndarray
    bbox: np.ndarray
    dev_sum: np.ndarray
    moment: np.ndarray
    r_abs_max: np.ndarray
    r_abs_sum: np.ndarray
    r_sq_sum: np.ndarray
    info: dict = field(default_factory=dict)
    residual: np.ndarray | None = field(default=None, repr=False)


_FIT_ARRAYS = (("status", np.int32, 1), ("n_points", np.int64, 1), ("center", np.int32, 3), ("normal", np.float64, 3),
               ("bbox", np.int32, 6), ("dev_sum", np.int64, 3), ("moment", np.int64, 6), ("r_abs_max", np.int32, 1),
               ("r_abs_sum", np.int64, 1), ("r_sq_sum", np.int64, 1))


def _take_fits(L, out, residual) -> PlaneFits:
    """Copy a bs_plane_fits into numpy arrays and release it."""
    n = out.n_planes
    try:
        arrs = _copy_arrays(out, _FIT_ARRAYS, n)
        info = {k: getattr(out, k) for k in ("ms_sums", "ms_moments", "ms_solve", "ms_residuals")}
        return PlaneFits(n, info=info, residual=residual, **arrs)
    finally:
        _free(L, out)


def plane_fit_apply(fits: PlaneFits, normal, center):
    """New (normal f64 [n_planes][3], center int32 [n_planes][3]) tables (bs_plane_fit_apply): the rows of the fitted
    planes (status 0) taken from `fits`, the other rows from the tables given (those of segment()'s planes)."""
    n = fits.n_planes
    nrm = np.array(normal, dtype=np.float64).reshape(-1, 3)  # (copies)
    ctr = np.array(center, dtype=np.int32).reshape(-1, 3)
    if len(nrm) != n or len(ctr) != n:
        raise ValueError("plane_fit_apply: normal and center must have one row per plane")
    st = _lib.PlaneFits()
    st.n_planes = n
    keep = []
    for name, cols, dt in (("status", 1, np.int32), ("normal", 3, np.float64), ("center", 3, np.int32)):
        a = np.ascontiguousarray(getattr(fits, name), dtype=dt)
        if a.size != n * cols:
            raise ValueError(f"PlaneFits.{name} must have {n * cols} entries")
        keep.append(a if n else np.zeros(cols, dt))  # (never a null pointer)
        setattr(st, name, keep[-1].ctypes.data_as(C.POINTER(C.c_double if dt == np.float64 else C.c_int32)))
    rc = _lib.load().bs_plane_fit_apply(C.byref(st), (nrm if n else np.zeros(3)).ctypes.data,
                                        (ctr if n else np.zeros(3, np.int32)).ctypes.data)
    if rc != 0:
        raise BsError(rc, "plane_fit_apply")
    return nrm, ctr


def roof_homes(normal, plane_building, votes_in, votes_total, min_normal_z=0.5) -> np.ndarray:
    """home int32 [n_planes] (bs_roof_homes): the building a plane may be a roof in -- its plane_building if the
    normal's z is at least min_normal_z and the building holds more than half of the plane's points -- or -1."""
    pb = np.ascontiguousarray(plane_building, dtype=np.int32).reshape(-1)
    n = len(pb)
    nrm = np.ascontiguousarray(normal, dtype=np.float64).reshape(-1, 3)
    vin = np.ascontiguousarray(votes_in, dtype=np.int64).reshape(-1)
    vtot = np.ascontiguousarray(votes_total, dtype=np.int64).reshape(-1)
    if len(nrm) != n or len(vin) != n or len(vtot) != n:
        raise ValueError("roof_homes: one entry per plane in every array")
    home = np.full(n, -1, dtype=np.int32)
    rc = _lib.load().bs_roof_homes(nrm.ctypes.data, pb.ctypes.data, vin.ctypes.data, vtot.ctypes.data, n,
                                   float(min_normal_z), home.ctypes.data)
    if rc != 0:
        raise BsError(rc, "roof_homes")
    return home


def write_roofs_obj(roofs: Roofs, bmap, path, origin=None, roof=None, normal=None, center=None, bin=None):
    """Roof OBJ in millimetres through the library's writer (bs_roofs_write_obj; the format is written down in
    include/bs_api.h): one quad per run of pixels with the same building and roof plane, its corners on the plane
    (clamped to the plane's supporting points).  roof / normal / center / bin default to what `roofs` carries."""
    roof = roofs.roof if roof is None else roof
    if roof is None:
        raise ValueError("write_roofs_obj: the roof image is on the device: pass roof=")
    roof = np.ascontiguousarray(roof, dtype=np.int32)
    bmap = np.ascontiguousarray(bmap, dtype=np.int32)
    if roof.ndim != 2 or bmap.shape != roof.shape:
        raise ValueError("write_roofs_obj: roof and bmap must be [height][width] of the same size")
    n = roofs.n_planes
    nrm = np.ascontiguousarray(roofs.normal if normal is None else normal, dtype=np.float64).reshape(-1, 3)
    ctr = np.ascontiguousarray(roofs.center if center is None else center, dtype=np.int32).reshape(-1, 3)
    if len(nrm) != n or len(ctr) != n:
        raise ValueError("write_roofs_obj: normal and center must have one entry per plane")
    st = _lib.Roofs()
    st.n_planes, st.width, st.height = n, roof.shape[1], roof.shape[0]
    keep = []
    for name, dt in (("pixels", np.int64), ("z_min", np.int32), ("z_max", np.int32)):
        a = np.ascontiguousarray(getattr(roofs, name), dtype=dt)
        if a.shape != (n,):
            raise ValueError(f"Roofs.{name} must be [{n}]")
        keep.append(a if n else np.zeros(1, dt))
        setattr(st, name, keep[-1].ctypes.data_as(C.POINTER(C.c_int32 if dt == np.int32 else C.c_int64)))
    h, w = roof.shape
    _write_obj("bs_roofs_write_obj", path, "a roof value above n_planes", roof, bmap, w, h, C.byref(st), _ptr0(nrm), _ptr0(ctr),
               int(roofs.bin if bin is None else bin), _origin(origin))


@dataclass
class Solids:
    """bs_solids: the totals, the per-building figures, and the mesh (None after solids_dev: it is written by
    solids_emit_dev).  vertex is [n_vertices][4] int32 {X, Y, Z, building} in millimetres, face f has the vertices
    face_index[face_offset[f] : face_offset[f + 1]]; face_kind 0 top, 1 floor, 2 wall.  The volume of building c in
    mm^3 is volume6[c] * bin^2 / 6.  base: the per-building table the Solids were built under (set_building_bases), None
    for the scalar base_z."""
    n_buildings: int
    width: int
    image_height: int
    bin: int
    base_z: int
    n_pixels: int
    n_vertices: int
    n_faces: int
    n_indices: int
    n_wall_faces: int
    n_crossing_walls: int
    total_volume6: int
    pixels: np.ndarray
    vertices: np.ndarray
    faces: np.ndarray
    wall_faces: np.ndarray
    crossing_walls: np.ndarray
    top_min: np.ndarray
    top_max: np.ndarray
    volume6: np.ndarray
    info: dict = field(default_factory=dict)
    top: np.ndarray | None = field(default=None, repr=False)
    vertex: np.ndarray | None = field(default=None, repr=False)
    face_offset: np.ndarray | None = field(default=None, repr=False)
    face_index: np.ndarray | None = field(default=None, repr=False)
    face_building: np.ndarray | None = field(default=None, repr=False)
    face_kind: np.ndarray | None = field(default=None, repr=False)
    base: np.ndarray | None = field(default=None, repr=False)


_SOLID_ARRAYS = (("pixels", np.int64, 1), ("vertices", np.int64, 1), ("faces", np.int64, 1), ("wall_faces", np.int64, 1),
                 ("crossing_walls", np.int64, 1), ("top_min", np.int32, 1), ("top_max", np.int32, 1), ("volume6", np.int64, 1))
_SOLID_TOTALS = ("bin", "base_z", "n_pixels", "n_vertices", "n_faces", "n_indices", "n_wall_faces", "n_crossing_walls",
                 "total_volume6")


def _solid_tables(normal, center, z_min, z_max):
    """(normal f64 [n][3], center int32 [n][3], z_min, z_max int32 [n]) as contiguous arrays"""
    z_min = np.ascontiguousarray(z_min, dtype=np.int32).reshape(-1)
    n = len(z_min)
    z_max = np.ascontiguousarray(z_max, dtype=np.int32).reshape(-1)
    normal = np.ascontiguousarray(normal, dtype=np.float64).reshape(-1, 3)
    center = np.ascontiguousarray(center, dtype=np.int32).reshape(-1, 3)
    if len(normal) != n or len(center) != n or len(z_max) != n:
        raise ValueError("normal, center, z_min and z_max must have one entry per plane")
    return normal, center, z_min, z_max


def _solid_defaults(buildings, base_z, flat):
    """base_z and flat [n_buildings] int32 of Context.solids"""
    if base_z is None:
        if buildings is None:
            raise ValueError("solids: give base_z or the Buildings (for its ground_th)")
        base_z = int(buildings.ground_th)
    base_z = int(base_z)
    if flat is None:
        if buildings is None:
            raise ValueError("solids: give flat or the Buildings (for z_sum / n_above)")
        zs, na = np.asarray(buildings.z_sum, np.int64), np.asarray(buildings.n_above, np.int64)
        q = np.abs(zs) // np.maximum(na, 1) * np.sign(zs)  # truncated towards zero, as bs_buildings_write_obj divides
        flat = np.where(na > 0, q, base_z)
    return base_z, np.ascontiguousarray(flat, dtype=np.int32).reshape(-1)


def _solid_inputs(who, bmap, roofs, buildings, base_z, flat):
    """(bmap, roof image, base_z, flat, tables) of Context.solids and Context.generalise_roofs"""
    bmap = np.ascontiguousarray(bmap, dtype=np.int32)
    roof = np.ascontiguousarray(_host_image(who, roofs.roof, "roof", who + "_dev"), dtype=np.int32)
    if bmap.ndim != 2 or roof.shape != bmap.shape:
        raise ValueError(f"{who}: bmap and roofs.roof must be [height][width] of the same size")
    base_z, flat = _solid_defaults(buildings, base_z, flat)
    return bmap, roof, base_z, flat, _solid_tables(roofs.normal, roofs.center, roofs.z_min, roofs.z_max)


def _take_mesh(out):
    """the five mesh arrays of a bs_solids or a bs_poly_solids"""
    nv, nf, ni = out.n_vertices, out.n_faces, out.n_indices
    return dict(vertex=_copy(out.vertex, (nv, 4), np.int32), face_offset=_copy(out.face_offset, (nf + 1,), np.int32),
                face_index=_copy(out.face_index, (ni,), np.int32), face_building=_copy(out.face_building, (nf,), np.int32),
                face_kind=_copy(out.face_kind, (nf,), np.uint8))


def _take_solids(L, out, top, mesh) -> Solids:
    """Copy a bs_solids into numpy arrays and release it."""
    n = out.n_buildings
    try:
        arrs = _copy_arrays(out, _SOLID_ARRAYS, n)
        if mesh:
            arrs.update(_take_mesh(out))
        info = {k: getattr(out, k) for k in ("ms_tops", "ms_vertices", "ms_faces", "ms_figures", "ms_scans",
                                             "ms_emit_vertices", "ms_emit_faces")}
        return Solids(n, out.width, out.height, *[getattr(out, k) for k in _SOLID_TOTALS], info=info, top=top, **arrs)
    finally:
        _free(L, out)


def write_solids_obj(solids, path, origin=None):
    """The mesh as an OBJ in millimetres through the library's writer (bs_solids_write_obj; the format is written down
    in include/bs_api.h): all vertices, then per building its faces.  `solids` is a Solids (or anything with vertex,
    face_offset, face_index, face_building and n_buildings); origin: the shift that was subtracted from the cloud."""
    if solids.vertex is None:
        raise ValueError("write_solids_obj: the mesh is on the device")
    v = np.ascontiguousarray(solids.vertex, dtype=np.int32).reshape(-1, 4)
    off = np.ascontiguousarray(solids.face_offset, dtype=np.int32).reshape(-1)
    idx = np.ascontiguousarray(solids.face_index, dtype=np.int32).reshape(-1)
    fb = np.ascontiguousarray(solids.face_building, dtype=np.int32).reshape(-1)
    if len(off) != len(fb) + 1 or (len(off) and int(off[-1]) != len(idx)):
        raise ValueError("write_solids_obj: face_offset must be [n_faces + 1] and end at len(face_index)")
    _write_obj("bs_solids_write_obj", path, "the mesh arrays do not fit each other", _ptr0(v), len(v), off, _ptr0(idx), _ptr0(fb),
               len(fb), int(solids.n_buildings), _origin(origin))


@dataclass
class RoofGeneralise:
    """bs_roof_generalise: rounds (applied evaluations), converged, the in / out totals, the per-evaluation arrays
    [rounds + 1] (eval_*), the per-plane pixel counts [n_planes + 1] (entry 0 = unroofed) and the per-building figures as
    include/bs_api.h names them; roof is the new roof image (None after generalise_roofs_dev) and roofs the Roofs over it."""
    width: int
    image_height: int
    n_buildings: int
    n_planes: int
    rounds: int
    converged: int
    n_facets_in: int
    n_facets_out: int
    n_edges_in: int
    n_edges_out: int
    n_flat_in: int
    n_flat_out: int
    n_small_in: int
    n_small_out: int
    pixels_changed: int
    pixels_roofed: int
    eval_facets: np.ndarray
    eval_movers: np.ndarray
    eval_movers_small: np.ndarray
    eval_movers_flat: np.ndarray
    eval_longest_chain: np.ndarray
    plane_pixels_in: np.ndarray
    plane_pixels_out: np.ndarray
    building_facets_in: np.ndarray
    building_facets_out: np.ndarray
    building_pixels_changed: np.ndarray
    building_sum_abs_dtop: np.ndarray
    building_max_abs_dtop: np.ndarray
    info: dict = field(default_factory=dict)
    roof: np.ndarray | None = field(default=None, repr=False)
    roofs: "Roofs | None" = field(default=None, repr=False)


_GEN_ARRAYS = tuple(_rows(g, np.int64) for g in (_lib.GEN_EVAL, _lib.GEN_PLANE, _lib.GEN_BUILDING))


def _take_roof_generalise(L, out, roof) -> RoofGeneralise:
    """Copy a bs_roof_generalise into numpy arrays and release it."""
    try:
        arrs = {}
        for group, n in zip(_GEN_ARRAYS, (out.rounds + 1, out.n_planes + 1, out.n_buildings)):
            arrs.update(_copy_arrays(out, group, n))
        info = {k: getattr(out, k) for k in _lib.GEN_MS}
        return RoofGeneralise(out.width, out.height, out.n_buildings, out.n_planes, out.rounds, out.converged,
                              *[getattr(out, k) for k in _lib.GEN_SCALARS], info=info, roof=roof, **arrs)
    finally:
        _free(L, out)


@dataclass
class RoofFacets:
    """bs_roof_facets: the facet image (None after roof_facets_dev), the totals, the per-facet arrays (facet_*) and the
    per-edge arrays (edge_*) as include/bs_api.h names them.  Facets are numbered by ascending start pixel, edges by
    ascending (facet_lo, facet_hi)."""
    width: int
    image_height: int
    n_facets: int
    n_edges: int
    n_pixels: int
    n_border: int
    facet_building: np.ndarray
    facet_plane: np.ndarray
    facet_start_xy: np.ndarray
    facet_pixels: np.ndarray
    facet_bbox: np.ndarray
    facet_inner_edges: np.ndarray
    facet_outer_edges: np.ndarray
    facet_top_min: np.ndarray
    facet_top_max: np.ndarray
    facet_top_sum: np.ndarray
    edge_facet: np.ndarray
    edge_building: np.ndarray
    edge_length: np.ndarray
    edge_n_dir0: np.ndarray
    edge_n_step: np.ndarray
    edge_step_abs_sum: np.ndarray
    edge_step_abs_max: np.ndarray
    edge_rise_sum: np.ndarray
    edge_bend_sum: np.ndarray
    edge_z_min: np.ndarray
    edge_z_max: np.ndarray
    edge_bbox: np.ndarray
    info: dict = field(default_factory=dict)
    facet: np.ndarray | None = field(default=None, repr=False)


# (name, dtype, columns) of the per-facet and per-edge arrays of bs_roof_facets
_FACET_ARRAYS = (("facet_building", np.int32, 1), ("facet_plane", np.int32, 1), ("facet_start_xy", np.int32, 2),
                 ("facet_pixels", np.int64, 1), ("facet_bbox", np.int32, 4), ("facet_inner_edges", np.int64, 1),
                 ("facet_outer_edges", np.int64, 1), ("facet_top_min", np.int32, 1), ("facet_top_max", np.int32, 1),
                 ("facet_top_sum", np.int64, 1))
_EDGE_ARRAYS = (("edge_facet", np.int32, 2), ("edge_building", np.int32, 1), ("edge_length", np.int64, 1),
                ("edge_n_dir0", np.int64, 1), ("edge_n_step", np.int64, 1), ("edge_step_abs_sum", np.int64, 1),
                ("edge_step_abs_max", np.int64, 1), ("edge_rise_sum", np.int64, 1), ("edge_bend_sum", np.int64, 1),
                ("edge_z_min", np.int32, 1), ("edge_z_max", np.int32, 1), ("edge_bbox", np.int32, 4))


def _take_roof_facets(L, out, facet) -> RoofFacets:
    """Copy a bs_roof_facets into numpy arrays and release it."""
    try:
        arrs = {**_copy_arrays(out, _FACET_ARRAYS, out.n_facets), **_copy_arrays(out, _EDGE_ARRAYS, out.n_edges)}
        info = {k: getattr(out, k) for k in ("ms_label", "ms_number", "ms_figures", "ms_edges")}
        return RoofFacets(out.width, out.height, out.n_facets, out.n_edges, out.n_pixels, out.n_border, info=info,
                          facet=facet, **arrs)
    finally:
        _free(L, out)


def _roof_facets_struct(rf):
    """a bs_roof_facets over the arrays of a RoofFacets (or anything with its names), and the arrays to keep alive"""
    st, keep = _lib.RoofFacets(), []
    st.n_facets, st.n_edges = int(rf.n_facets), int(rf.n_edges)
    st.n_pixels, st.n_border = int(rf.n_pixels), int(rf.n_border)
    _fill(st, rf, "RoofFacets", _columns(_FACET_ARRAYS, st.n_facets) + _columns(_EDGE_ARRAYS, st.n_edges), keep)
    return st, keep


def roof_edge_kinds(rf, step_tol=200, bend_tol=0):
    """The kind of every edge of a RoofFacets (bs_roof_edge_kinds): uint8 [n_edges], 0 flat, 1 ridge, 2 valley, 3 step.
    step_tol: the mean height difference in millimetres along the border above which it is a step; bend_tol in the units
    of bend (twice the change of rise per pixel)."""
    st, keep = _roof_facets_struct(rf)
    kind = np.zeros(max(st.n_edges, 1), dtype=np.uint8)
    rc = _lib.load().bs_roof_edge_kinds(C.byref(st), int(step_tol), int(bend_tol), kind.ctypes.data)
    if rc != 0:
        raise BsError(rc, "roof_edge_kinds: a negative tolerance")
    return kind[:st.n_edges]


def write_roof_edges_obj(rf, bmap, top, path, bin, kinds=None, origin=None):
    """The border edges of a RoofFacets as an OBJ of line segments in millimetres through the library's writer
    (bs_roof_edges_write_obj; the format is written down in include/bs_api.h), one group per edge named by its kind.
    kinds defaults to roof_edge_kinds(rf); origin: the shift that was subtracted from the cloud."""
    if rf.facet is None:
        raise ValueError("write_roof_edges_obj: the facet image is on the device")
    facet = np.ascontiguousarray(rf.facet, dtype=np.int32)
    bmap = np.ascontiguousarray(bmap, dtype=np.int32)
    top = np.ascontiguousarray(top, dtype=np.int32)
    if facet.ndim != 2 or bmap.shape != facet.shape or top.shape != facet.shape + (4,):
        raise ValueError("write_roof_edges_obj: facet and bmap must be [height][width] and top [height][width][4]")
    st, keep = _roof_facets_struct(rf)
    kinds = roof_edge_kinds(rf) if kinds is None else np.ascontiguousarray(kinds, dtype=np.uint8).reshape(-1)
    if len(kinds) != st.n_edges:
        raise ValueError("write_roof_edges_obj: kinds must be [n_edges]")
    h, w = facet.shape
    _write_obj("bs_roof_edges_write_obj", path, "a facet pair the RoofFacets do not list", facet, bmap, top, w, h, int(bin),
               C.byref(st), _ptr0(kinds), _origin(origin))


@dataclass
class Outlines:
    """bs_outlines: the totals, the per-ring arrays (ring_*), label_ring_offset and the vertices xy / z (None after
    facet_outlines_dev; z None without top) as include/bs_api.h names them.  Rings are listed by ascending (label, start);
    ring r has the vertices ring_offset[r] .. ring_offset[r + 1]."""
    width: int
    image_height: int
    n_labels: int
    n_half: int
    n_rings: int
    n_vertices: int
    ring_label: np.ndarray
    ring_start: np.ndarray
    ring_length: np.ndarray
    ring_vertices: np.ndarray
    ring_area2: np.ndarray
    ring_bbox: np.ndarray
    ring_offset: np.ndarray
    label_ring_offset: np.ndarray
    has_z: bool = False
    info: dict = field(default_factory=dict)
    xy: np.ndarray | None = field(default=None, repr=False)
    z: np.ndarray | None = field(default=None, repr=False)


# (name, dtype, columns) of the per-ring arrays of bs_outlines
_RING_ARRAYS = (("ring_label", np.int32, 1), ("ring_start", np.int32, 1), ("ring_length", np.int64, 1),
                ("ring_vertices", np.int64, 1), ("ring_area2", np.int64, 1), ("ring_bbox", np.int32, 4))


def _take_outlines(L, out, vertices) -> Outlines:
    """Copy a bs_outlines into numpy arrays and release it."""
    try:
        nr, nv = out.n_rings, out.n_vertices
        arrs = _copy_arrays(out, _RING_ARRAYS, nr)
        arrs["ring_offset"] = _copy(out.ring_offset, (nr + 1,), np.int64)
        arrs["label_ring_offset"] = _copy(out.label_ring_offset, (out.n_labels + 1,), np.int64)
        xy = _copy(out.xy, (nv, 2), np.int32) if vertices else None
        z = _copy(out.z, (nv,), np.int32) if vertices and out.has_z else None
        info = {k: getattr(out, k) for k in ("ms_halfedges", "ms_leaders", "ms_rank", "ms_rings", "ms_emit")}
        return Outlines(out.width, out.height, out.n_labels, out.n_half, nr, nv, has_z=bool(out.has_z), info=info, xy=xy, z=z,
                        **arrs)
    finally:
        _free(L, out)


def _outlines_struct(o):
    """a bs_outlines over the arrays of an Outlines (or anything with its names), and the arrays to keep alive"""
    st, keep = _lib.Outlines(), []
    st.n_labels, st.n_rings, st.n_vertices = int(o.n_labels), int(o.n_rings), int(o.n_vertices)
    st.n_half = int(o.n_half)
    st.has_z = int(o.z is not None)
    _fill(st, o, "Outlines", _columns(_RING_ARRAYS, st.n_rings) + [("ring_offset", np.int64, st.n_rings + 1),
          ("label_ring_offset", np.int64, st.n_labels + 1), ("xy", np.int32, 2 * st.n_vertices)] +
          [("z", np.int32, st.n_vertices)] * st.has_z, keep)
    return st, keep


def write_outlines_obj(outlines, path, bin, origin=None):
    """The rings of an Outlines as an OBJ of closed polylines in millimetres through the library's writer
    (bs_outlines_write_obj; the format is written down in include/bs_api.h), one group per ring.  origin: the shift that
    was subtracted from the cloud."""
    if outlines.xy is None:
        raise ValueError("write_outlines_obj: the vertices are on the device")
    st, keep = _outlines_struct(outlines)
    _write_obj("bs_outlines_write_obj", path, "the ring arrays do not fit each other", C.byref(st), int(bin), _origin(origin))


@dataclass
class SimpleOutlines:
    """bs_simple_outlines: the totals, the per-ring arrays (s_ring_*, and ring_label / ring_area2 / label_ring_offset of the
    plain outlines) and the kept vertices sxy / sz / s_right / s_flag (None after simplified_outlines_dev; sz None without
    top) as include/bs_api.h names them.  Ring r has the vertices s_ring_offset[r] .. s_ring_offset[r + 1]."""
    width: int
    image_height: int
    n_labels: int
    tol_num: int
    tol_den: int
    n_rings: int
    n_nodes: int
    n_junction_nodes: int
    n_arcs: int
    n_svertices: int
    rounds: int
    max_arc_nodes: int
    ring_label: np.ndarray
    ring_area2: np.ndarray
    s_ring_vertices: np.ndarray
    s_ring_area2: np.ndarray
    s_ring_arcs: np.ndarray
    s_ring_offset: np.ndarray
    label_ring_offset: np.ndarray
    has_z: bool = False
    info: dict = field(default_factory=dict)
    sxy: np.ndarray | None = field(default=None, repr=False)
    sz: np.ndarray | None = field(default=None, repr=False)
    s_right: np.ndarray | None = field(default=None, repr=False)
    s_flag: np.ndarray | None = field(default=None, repr=False)


_SIMPLE_RING_ARRAYS = (("ring_label", np.int32, 1), ("ring_area2", np.int64, 1), ("s_ring_vertices", np.int64, 1),
                       ("s_ring_area2", np.int64, 1), ("s_ring_arcs", np.int64, 1))
_SIMPLE_TOTALS = ("n_rings", "n_nodes", "n_junction_nodes", "n_arcs", "n_svertices", "rounds", "max_arc_nodes")


_SIMPLE_MS = ("ms_outlines", "ms_nodes", "ms_placing", "ms_arcs", "ms_rounds", "ms_rings", "ms_emit")


def _take_kept_outlines(L, out, vertices, cls, ms, totals=()):
    """Copy a bs_simple_outlines or a bs_clean_outlines into the dataclass cls (its info: the fields ms; the totals it has
    beyond the simplified ones: totals) and release it."""
    try:
        nr, nv = out.n_rings, out.n_svertices
        arrs = _copy_arrays(out, _SIMPLE_RING_ARRAYS, nr)
        arrs["s_ring_offset"] = _copy(out.s_ring_offset, (nr + 1,), np.int64)
        arrs["label_ring_offset"] = _copy(out.label_ring_offset, (out.n_labels + 1,), np.int64)
        v = dict(sxy=None, sz=None, s_right=None, s_flag=None)
        if vertices:
            v.update(sxy=_copy(out.sxy, (nv, 2), np.int32), s_right=_copy(out.s_right, (nv,), np.int32),
                     s_flag=_copy(out.s_flag, (nv,), np.uint8), sz=_copy(out.sz, (nv,), np.int32) if out.has_z else None)
        return cls(out.width, out.height, out.n_labels, out.tol_num, out.tol_den, *[getattr(out, k) for k in _SIMPLE_TOTALS],
                   has_z=bool(out.has_z), info={k: getattr(out, k) for k in ms}, **arrs, **v,
                   **{k: getattr(out, k) for k in totals})
    finally:
        _free(L, out)


def _take_simple_outlines(L, out, vertices) -> SimpleOutlines:
    """Copy a bs_simple_outlines into numpy arrays and release it."""
    return _take_kept_outlines(L, out, vertices, SimpleOutlines, _SIMPLE_MS)


@dataclass
class CleanOutlines(SimpleOutlines):
    """bs_clean_outlines: a SimpleOutlines over the repaired kept set (s_flag bit 2: kept by the repair, bit 3: still
    marked) with the figures of the conflict check and repair as include/bs_api.h names them."""
    max_rounds: int = -1
    cell_log2: int = 0
    n_svertices_before: int = 0
    n_marked_first: int = 0
    n_marked_left: int = 0
    n_forced: int = 0
    repair_rounds: int = 0
    n_entries: int = 0
    max_cell_entries: int = 0


@dataclass
class OutlineSweeps:
    """bs_outline_sweeps: the figures of the sweep detection of a clean count as include/bs_api.h names them."""
    mode: int = 0
    wave_cap: int = 0
    n_lens_segments_first: int = 0
    n_sweeping_first: int = 0
    n_sweeping_only_first: int = 0
    n_swept_pairs_first: int = 0
    max_abs_winding: int = 0
    sweep_rounds: int = 0
    n_sweeping_left: int = 0
    n_items_first: int = 0
    n_items_swapped_first: int = 0
    n_candidates_first: int = 0
    n_exact_first: int = 0
    n_exact_wave_first: int = 0
    n_rejected_first: int = 0
    ms_sweep: float = 0.0


_CLEAN_TOTALS = ("max_rounds", "cell_log2", "n_svertices_before", "n_marked_first", "n_marked_left", "n_forced", "repair_rounds",
                 "n_entries", "max_cell_entries")


def _take_clean_outlines(L, out, vertices) -> CleanOutlines:
    """Copy a bs_clean_outlines into numpy arrays and release it."""
    return _take_kept_outlines(L, out, vertices, CleanOutlines, ("ms_simplify", "ms_detect", "ms_repair", "ms_rings", "ms_emit"),
                               _CLEAN_TOTALS)


def _kept_outlines_struct(st, o, what, scalars=()):
    """the bs_simple_outlines or bs_clean_outlines `st` over what its writer reads of o, and the arrays to keep alive"""
    for k in ("n_labels", "n_rings", "n_svertices", "tol_num", "tol_den") + scalars:
        setattr(st, k, int(getattr(o, k)))
    st.has_z = int(o.sz is not None)
    return st, _fill(st, o, what, [("ring_label", np.int32, st.n_rings), ("ring_area2", np.int64, st.n_rings),
                                   ("s_ring_offset", np.int64, st.n_rings + 1), ("label_ring_offset", np.int64, st.n_labels + 1),
                                   ("sxy", np.int32, 2 * st.n_svertices)] + [("sz", np.int32, st.n_svertices)] * st.has_z, [])


def write_clean_outlines_obj(clean, path, bin, origin=None):
    """The rings of a CleanOutlines as an OBJ through the library's writer (bs_clean_outlines_write_obj)."""
    if clean.sxy is None:
        raise ValueError("write_clean_outlines_obj: the vertices are on the device")
    st, keep = _kept_outlines_struct(_lib.CleanOutlines(), clean, "CleanOutlines", ("repair_rounds", "n_forced"))
    _write_obj("bs_clean_outlines_write_obj", path, "the ring arrays do not fit each other", C.byref(st), int(bin), _origin(origin))


@dataclass
class OutlineTriangles:
    """bs_outline_triangles: the triangles of every label over the clean vertices, tri_offset per label, the status, area
    and ear tests of every label, the bridge (M, V) of every hole, and the totals as include/bs_api.h names them."""
    n_labels: int
    n_rings: int
    n_svertices: int
    n_triangles: int
    n_failed_labels: int
    n_bridges: int
    n_tests: int
    max_label_occurrences: int
    n_labels_wave: int
    n_labels_lds: int
    n_labels_global: int
    wave_cap: int
    lds_cap: int
    tri_offset: np.ndarray
    label_status: np.ndarray
    label_area2: np.ndarray
    label_tests: np.ndarray
    bridge: np.ndarray
    info: dict = field(default_factory=dict)
    tri: np.ndarray | None = field(default=None, repr=False)


_TRI_TOTALS = ("n_labels", "n_rings", "n_svertices", "n_triangles", "n_failed_labels", "n_bridges", "n_tests",
               "max_label_occurrences", "n_labels_wave", "n_labels_lds", "n_labels_global", "wave_cap", "lds_cap")
_TRI_LABEL_ARRAYS = (("label_status", np.int32, 1), ("label_area2", np.int64, 1), ("label_tests", np.int64, 1))


def _take_outline_triangles(L, out, triangles) -> OutlineTriangles:
    """Copy a bs_outline_triangles into numpy arrays and release it."""
    try:
        nl = out.n_labels
        info = {k: getattr(out, k) for k in ("ms_clean", "ms_prologue", "ms_wave", "ms_lds", "ms_global", "ms_emit")}
        return OutlineTriangles(*[getattr(out, k) for k in _TRI_TOTALS], tri_offset=_copy(out.tri_offset, (nl + 1,), np.int64),
                                **_copy_arrays(out, _TRI_LABEL_ARRAYS, nl), bridge=_copy(out.bridge, (out.n_rings, 2), np.int32),
                                info=info, tri=_copy(out.tri, (out.n_triangles, 3), np.int32) if triangles else None)
    finally:
        _free(L, out)


def write_outline_triangles_obj(tri, clean, path, bin, origin=None):
    """The mesh of an OutlineTriangles over the vertices of its CleanOutlines as an OBJ through the library's writer
    (bs_outline_triangles_write_obj)."""
    if tri.tri is None or clean.sxy is None:
        raise ValueError("write_outline_triangles_obj: the triangles or the vertices are on the device")
    st, cl, keep = _lib.OutlineTriangles(), _lib.CleanOutlines(), []
    st.n_labels, st.n_svertices, st.n_triangles = int(tri.n_labels), int(tri.n_svertices), int(tri.n_triangles)
    st.n_failed_labels, st.n_bridges = int(tri.n_failed_labels), int(tri.n_bridges)
    cl.n_svertices, cl.has_z = int(clean.n_svertices), int(clean.sz is not None)
    _fill(st, tri, type(tri).__name__, [("tri_offset", np.int64, st.n_labels + 1), ("label_status", np.int32, st.n_labels),
                                        ("tri", np.int32, 3 * st.n_triangles)], keep)
    _fill(cl, clean, type(clean).__name__, [("sxy", np.int32, 2 * cl.n_svertices)] + [("sz", np.int32, cl.n_svertices)] * cl.has_z,
          keep)
    _write_obj("bs_outline_triangles_write_obj", path, "the arrays do not fit each other", C.byref(st), C.byref(cl), int(bin),
               _origin(origin))


@dataclass
class PolySolids:
    """bs_poly_solids: the totals, the per-building figures (status 0 closed / 1 open, labels, vertices, faces, roof_faces,
    wall_faces, crossing_walls, max_wall_vertices, z_min, z_max, area2, volume6) and the mesh in the layout of Solids (None
    after poly_solids_dev: it is written by poly_solids_emit_dev), which write_solids_obj writes.  The volume of building c
    in mm^3 is volume6[c] * bin^2 / 6."""
    n_buildings: int
    n_labels: int
    bin: int
    base_z: int
    fig_cap: int
    n_open_buildings: int
    n_vertices: int
    n_faces: int
    n_indices: int
    n_roof_faces: int
    n_wall_faces: int
    n_crossing_walls: int
    max_wall_vertices_all: int
    total_area2: int
    total_volume6: int
    status: np.ndarray
    labels: np.ndarray
    vertices: np.ndarray
    faces: np.ndarray
    roof_faces: np.ndarray
    wall_faces: np.ndarray
    crossing_walls: np.ndarray
    max_wall_vertices: np.ndarray
    z_min: np.ndarray
    z_max: np.ndarray
    area2: np.ndarray
    volume6: np.ndarray
    info: dict = field(default_factory=dict)
    vertex: np.ndarray | None = field(default=None, repr=False)
    face_offset: np.ndarray | None = field(default=None, repr=False)
    face_index: np.ndarray | None = field(default=None, repr=False)
    face_building: np.ndarray | None = field(default=None, repr=False)
    face_kind: np.ndarray | None = field(default=None, repr=False)


_POLY_ARRAYS = tuple((k, np.dtype(ct), 1) for k, ct in _lib.POLY_FIGURES)


def _take_poly_solids(L, out, mesh) -> PolySolids:
    """Copy a bs_poly_solids into numpy arrays and release it."""
    n = out.n_buildings
    try:
        arrs = _copy_arrays(out, _POLY_ARRAYS, n)
        if mesh:
            arrs.update(_take_mesh(out))
        info = {k: getattr(out, k) for k in _lib.POLY_MS}
        return PolySolids(n, out.n_labels, out.bin, out.base_z, out.fig_cap, *[getattr(out, k) for k in _lib.POLY_TOTALS],
                          info=info, **arrs)
    finally:
        _free(L, out)


@dataclass
class ModelRaster:
    """bs_model_raster: the totals, the per-label figures (pixels, model_pixels, kept, multi, err_pixels, sum_abs_e2,
    max_abs_e2, sq_lo, sq_hi; the sum of e2 squared of label l is sq_hi[l] * 2^32 + sq_lo[l]) and the three images: model
    (the label the model puts on the pixel, -1: none), cover (the triangles that cover its centre), mz2 (twice the model's
    height at the centre, INT32_MIN where none).  The images are None after model_raster_dev."""
    width: int
    height: int
    n_labels: int
    fig_cap: int
    chunk: int
    n_triangles: int
    total_pixels: int
    total_model_pixels: int
    total_kept: int
    total_err_pixels: int
    total_sum_abs_e2: int
    max_abs_e2_all: int
    total_sq_lo: int
    total_sq_hi: int
    n_uncovered: int
    n_spill: int
    n_moved: int
    n_multi: int
    sum_cover: int
    n_rows: int
    n_items: int
    n_empty_spans: int
    max_span: int
    pixels: np.ndarray
    model_pixels: np.ndarray
    kept: np.ndarray
    multi: np.ndarray
    err_pixels: np.ndarray
    sum_abs_e2: np.ndarray
    max_abs_e2: np.ndarray
    sq_lo: np.ndarray
    sq_hi: np.ndarray
    info: dict = field(default_factory=dict)
    model: np.ndarray | None = field(default=None, repr=False)
    cover: np.ndarray | None = field(default=None, repr=False)
    mz2: np.ndarray | None = field(default=None, repr=False)


_MRASTER_ARRAYS = _rows(_lib.MRASTER_FIGURES, np.int64)


def _take_model_raster(L, out, model=None, cover=None, mz2=None) -> ModelRaster:
    """Copy a bs_model_raster into numpy arrays and release it."""
    n = out.n_labels
    try:
        arrs = _copy_arrays(out, _MRASTER_ARRAYS, n)
        info = {k: getattr(out, k) for k in _lib.MRASTER_MS}
        return ModelRaster(out.width, out.height, n, out.fig_cap, out.chunk, *[getattr(out, k) for k in _lib.MRASTER_TOTALS],
                           info=info, model=model, cover=cover, mz2=mz2, **arrs)
    finally:
        _free(L, out)


@dataclass
class ModelFidelity:
    """Per building, from a ModelRaster and the building of every label.  lost: pixels of its labels that the model does
    not give to the same label; gained: pixels the model gives to one of its labels that the image does not; twice: pixels
    of its labels in the model that more than one triangle covers (an overlap in plan).  Over the pixels that are labelled
    in both (err_pixels): the mean and the maximum absolute height error and the RMSE, in the unit of top (millimetres)."""
    n_buildings: int
    pixels: np.ndarray
    lost: np.ndarray
    gained: np.ndarray
    twice: np.ndarray
    err_pixels: np.ndarray
    mean_abs_mm: np.ndarray
    max_abs_mm: np.ndarray
    rmse_mm: np.ndarray


def _by_building(who, label_building, n_labels, n_buildings):
    """(label_building int64 [n_labels], n_buildings, add: the per-label figures v added up by building) of the fidelities"""
    lb = np.ascontiguousarray(label_building, dtype=np.int64).reshape(-1)
    if len(lb) != n_labels:
        raise ValueError(f"{who}: label_building must have one entry per label")
    nb = (int(lb.max()) + 1 if len(lb) else 0) if n_buildings is None else int(n_buildings)
    if len(lb) and (lb.min() < 0 or lb.max() >= nb):
        raise ValueError(f"{who}: a label_building value outside 0 .. n_buildings - 1")

    def add(v):
        s = np.zeros(nb, np.int64)
        np.add.at(s, lb, v)
        return s

    return lb, nb, add


def model_fidelity_of(raster, label_building, n_buildings=None) -> ModelFidelity:
    """The per-label figures of a ModelRaster added up by building (host only; Python integers for the sum of squares)."""
    lb, nb, add = _by_building("model_fidelity_of", label_building, raster.n_labels, n_buildings)
    pixels, kept, errp = add(raster.pixels), add(raster.kept), add(raster.err_pixels)
    mx = np.zeros(nb, np.int64)
    np.maximum.at(mx, lb, raster.max_abs_e2)
    sq = [0] * nb
    for l, c in enumerate(lb.tolist()):
        sq[c] += (int(raster.sq_hi[l]) << 32) + int(raster.sq_lo[l])
    n = np.maximum(errp, 1)
    rmse = np.array([(sq[c] / 4 / int(n[c])) ** 0.5 for c in range(nb)], np.float64)
    return ModelFidelity(nb, pixels, pixels - kept, add(raster.model_pixels) - kept, add(raster.multi), errp,
                         add(raster.sum_abs_e2) / 2.0 / n, mx / 2.0, rmse)


NO_CLIP2 = (1 << 31) - 1  # clip2 of a call without clipping: no |r2| reaches it


def _clip2(clip2):
    if clip2 is None:
        return NO_CLIP2
    c = int(clip2)
    if c != clip2 or c > NO_CLIP2:
        raise ValueError("clip2 must be a whole number below 2^31 or None")
    return c


def _plane_pair(who, plane_idx, label_plane, n, nl):
    if (plane_idx is None) != (label_plane is None):
        raise ValueError(f"{who}: plane_idx and label_plane come together or not at all")
    if plane_idx is None:
        return None, None
    pi = np.ascontiguousarray(plane_idx, dtype=np.int32).reshape(-1)
    lp = np.ascontiguousarray(label_plane, dtype=np.int32).reshape(-1)
    if len(pi) != n or len(lp) != nl:
        raise ValueError(f"{who}: plane_idx must have one entry per point and label_plane one per label")
    return pi, (lp if nl else np.zeros(1, np.int32))


@dataclass
class PointResiduals:
    """bs_point_residuals: the totals, the per-label figures (points, multi, above, below, and over the inliers in_points,
    sum_r2, sum_abs_r2, max_abs_r2, sq_lo, sq_hi; plane_points, plane_in; the sum of r2 squared of label l is
    sq_hi[l] * 2^32 + sq_lo[l]) and the three per-point arrays: label (the label of the triangle over the point, -1: none),
    r2 (twice the point's height above the model, INT32_MIN where none), cover (the triangles that cover it).  The arrays
    are None after point_residuals_dev."""
    width: int
    height: int
    n_labels: int
    bin: int
    clip2: int
    fig_cap: int
    chunk: int
    grid: int
    n_points: int
    n_triangles: int
    total_points: int
    total_above: int
    total_below: int
    total_in_points: int
    total_sum_r2: int
    total_sum_abs_r2: int
    max_abs_r2_all: int
    total_sq_lo: int
    total_sq_hi: int
    total_plane_points: int
    total_plane_in: int
    n_uncovered: int
    n_multi: int
    n_rows: int
    n_items: int
    max_list: int
    n_empty_pixel: int
    n_height_wide: int
    points: np.ndarray
    multi: np.ndarray
    above: np.ndarray
    below: np.ndarray
    in_points: np.ndarray
    sum_r2: np.ndarray
    sum_abs_r2: np.ndarray
    max_abs_r2: np.ndarray
    sq_lo: np.ndarray
    sq_hi: np.ndarray
    plane_points: np.ndarray
    plane_in: np.ndarray
    info: dict = field(default_factory=dict)
    label: np.ndarray | None = field(default=None, repr=False)
    r2: np.ndarray | None = field(default=None, repr=False)
    cover: np.ndarray | None = field(default=None, repr=False)


_PRESID_ARRAYS = _rows(_lib.PRESID_FIGURES, np.int64)


def _take_point_residuals(L, out, label=None, r2=None, cover=None) -> PointResiduals:
    """Copy a bs_point_residuals into numpy arrays and release it."""
    n = out.n_labels
    try:
        arrs = _copy_arrays(out, _PRESID_ARRAYS, n)
        info = {k: getattr(out, k) for k in _lib.PRESID_MS}
        return PointResiduals(*[getattr(out, k) for k in _lib.PRESID_HEAD + _lib.PRESID_TOTALS], info=info, label=label, r2=r2,
                              cover=cover, **arrs)
    finally:
        _free(L, out)


@dataclass
class PointFidelity:
    """Per building, from a PointResiduals and the building of every label.  points: the points over one of its labels;
    inlier_share, above_share, below_share: the parts of them within the clip, above and below it; over the inliers the
    bias (the signed mean residual), the mean absolute residual, the maximum and the RMSE in millimetres; plane_share: the
    part of the points whose plane is the plane of their label, plane_in_share: the part of those that are inliers (both
    0 without a plane table).  A building without a point (or an inlier) has 0 in the shares (the means)."""
    n_buildings: int
    points: np.ndarray
    in_points: np.ndarray
    inlier_share: np.ndarray
    above_share: np.ndarray
    below_share: np.ndarray
    bias_mm: np.ndarray
    mean_abs_mm: np.ndarray
    max_abs_mm: np.ndarray
    rmse_mm: np.ndarray
    plane_share: np.ndarray
    plane_in_share: np.ndarray


def point_fidelity_of(res, label_building, n_buildings=None) -> PointFidelity:
    """The per-label figures of a PointResiduals added up by building (host only; Python integers for the sum of squares)."""
    lb, nb, add = _by_building("point_fidelity_of", label_building, res.n_labels, n_buildings)
    points, inl, ppts = add(res.points), add(res.in_points), add(res.plane_points)
    mx = np.zeros(nb, np.int64)
    np.maximum.at(mx, lb, res.max_abs_r2)
    sq = [0] * nb
    for l, c in enumerate(lb.tolist()):
        sq[c] += (int(res.sq_hi[l]) << 32) + int(res.sq_lo[l])
    n, ni, npl = np.maximum(points, 1), np.maximum(inl, 1), np.maximum(ppts, 1)
    rmse = np.array([(sq[c] / 4 / int(ni[c])) ** 0.5 for c in range(nb)], np.float64)
    return PointFidelity(nb, points, inl, inl / n, add(res.above) / n, add(res.below) / n, add(res.sum_r2) / 2.0 / ni,
                         add(res.sum_abs_r2) / 2.0 / ni, mx / 2.0, rmse, ppts / n, add(res.plane_in) / npl)


def simplify_tolerance(tolerance_mm, bin):
    """The tolerance of the simplified outlines for a distance in millimetres on a raster of `bin` millimetres per pixel:
    tol2 = (tolerance_mm / bin)^2 as the reduced fraction (num, den) = (tolerance_mm^2, bin^2) / their gcd."""
    import math
    t, b = int(tolerance_mm), int(bin)
    if t != tolerance_mm or b != bin or t < 0 or b < 1:
        raise ValueError("simplify_tolerance: tolerance_mm must be a whole number >= 0 and bin a whole number >= 1")
    g = math.gcd(t * t, b * b)
    num, den = t * t // g, b * b // g
    if num >= 1 << 31 or den >= 1 << 31:
        raise ValueError("simplify_tolerance: the reduced fraction does not fit 31 bits")
    return num, den


def write_simple_outlines_obj(simple, path, bin, origin=None):
    """The rings of a SimpleOutlines as an OBJ of closed polylines in millimetres through the library's writer
    (bs_simple_outlines_write_obj; the format is written down in include/bs_api.h), one group per ring."""
    if simple.sxy is None:
        raise ValueError("write_simple_outlines_obj: the vertices are on the device")
    st, keep = _kept_outlines_struct(_lib.SimpleOutlines(), simple, "SimpleOutlines")
    _write_obj("bs_simple_outlines_write_obj", path, "the ring arrays do not fit each other", C.byref(st), int(bin),
               _origin(origin))


@dataclass
class Footprints:
    """Contours of bs_footprints in findContours' order, their contourArea / arcLength, and the stage info."""
    contours: list
    area: np.ndarray
    perimeter: np.ndarray
    width: int
    height: int
    info: dict = field(default_factory=dict)

    def kept(self, min_area=500.0, min_perimeter=100.0):
        """Indices the reference keeps for its drawn overlay (my_function.cpp:40)."""
        return [i for i in range(len(self.contours)) if self.area[i] > min_area and self.perimeter[i] > min_perimeter]


def _contours_struct(fp):
    """a bs_contours over the contours of a Footprints (without area and perimeter), and the arrays to keep alive"""
    n = len(fp.contours)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c) for c in fp.contours]) if n else []
    xy = np.ascontiguousarray(np.concatenate(fp.contours) if n else np.zeros((0, 2)), dtype=np.int32)
    c = Contours()
    c.n_contours, c.width, c.height = n, fp.width, fp.height
    c.offset = off.ctypes.data_as(C.POINTER(C.c_int64))
    c.xy = (xy if xy.size else _PAD).ctypes.data_as(C.POINTER(C.c_int32))
    return c, (off, xy)


def _contour_arrays(L, out: Contours):
    """(offset, xy, area, perimeter) copied out of a bs_contours, which is released."""
    n = out.n_contours
    try:
        off = _copy(out.offset, (n + 1,), np.int64) if out.offset else np.zeros(1, np.int64)
        xy = _copy(out.xy, (int(off[-1]), 2), np.int32)
        area, per = _copy(out.area, (n,), np.float64), _copy(out.perimeter, (n,), np.float64)
    finally:
        _free(L, out)
    return off, xy, area, per


def _take_contours(L, out: Contours, inf: FootprintInfo) -> Footprints:
    n, w, h = out.n_contours, out.width, out.height
    off, xy, area, per = _contour_arrays(L, out)
    return Footprints([xy[off[i]:off[i + 1]] for i in range(n)], area, per, w, h,
                      {k: getattr(inf, k) for k, _ in FootprintInfo._fields_})


def _take_contours_batch(L, out: Contours, inf: FootprintInfo, co, widths, heights) -> list:
    """One Footprints per tile of a bs_footprints_batch result: contours co[t] .. co[t+1] - 1."""
    off, xy, area, per = _contour_arrays(L, out)
    info = {k: getattr(inf, k) for k, _ in FootprintInfo._fields_}
    return [Footprints([xy[off[i]:off[i + 1]] for i in range(co[t], co[t + 1])], area[co[t]:co[t + 1]].copy(),
                       per[co[t]:co[t + 1]].copy(), int(widths[t]), int(heights[t]), info)
            for t in range(len(widths))]


def write_footprints_obj(fp: Footprints, path):
    """The reference's OBJ (my_function.cpp:64-131) through the library's writer (bs_contours_write_obj), so that
    Python and host/tmc3 --footprints= write the same bytes."""
    c, keep = _contours_struct(fp)
    _write_obj("bs_contours_write_obj", path, None, C.byref(c))


def _tile_offsets(tile_offset) -> np.ndarray:
    off = np.ascontiguousarray(tile_offset, dtype=np.int64)
    if off.ndim != 1 or len(off) < 2:
        raise ValueError("tile_offset must be a 1-D array of n_tiles + 1 >= 2 offsets")
    return off


def pack_tiles(tiles):
    """Pack a list of integer [n_t, 3] clouds into the batch layout of bs_segment_batch: (xyz int32 [N, 3], the
    concatenation, and tile_offset int64 [n_tiles + 1], tile t = rows tile_offset[t] .. tile_offset[t + 1] - 1)."""
    if isinstance(tiles, np.ndarray) or not hasattr(tiles, "__len__") or len(tiles) == 0:
        raise ValueError("tiles must be a non-empty list of [n, 3] arrays")
    arrs = []
    for t, a in enumerate(tiles):
        a = np.asarray(a)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"tile {t}: shape {a.shape}, expected [n, 3]")
        if a.shape[0] == 0:
            raise ValueError(f"tile {t} is empty")
        if not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"tile {t}: dtype {a.dtype}, expected integer coordinates (mm)")
        if a.dtype.itemsize > 4 or a.dtype == np.uint32:
            if a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max:
                raise ValueError(f"tile {t}: coordinates do not fit int32")
        arrs.append(a.astype(np.int32, copy=False))
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(a) for a in arrs])
    return np.ascontiguousarray(np.concatenate(arrs)), off


def shift_tiles_to_origin(xyz, tile_offset) -> np.ndarray:
    """Host form of bs_shift_tiles_to_origin_dev: every tile of a packed batch minus its own minimum."""
    off = _tile_offsets(tile_offset)
    if off[0] != 0 or (np.diff(off) <= 0).any() or off[-1] != len(xyz):
        raise ValueError("tile_offset must start at 0, rise strictly and end at len(xyz)")
    xyz = np.asarray(xyz, dtype=np.int64)
    mn = np.minimum.reduceat(xyz, off[:-1], axis=0)
    out = xyz - np.repeat(mn, np.diff(off), axis=0)
    if out.max(initial=0) > np.iinfo(np.int32).max:
        raise ValueError("a tile's extent does not fit int32")
    return out.astype(np.int32)


def _tile_extents(extents, n_tiles) -> np.ndarray:
    ext = np.asarray(extents)
    if ext.shape != (n_tiles, 3):
        raise ValueError(f"extents must be [n_tiles, 3] = [{n_tiles}, 3], got {ext.shape}")
    if not np.issubdtype(ext.dtype, np.integer):
        raise TypeError(f"extents: dtype {ext.dtype}, expected integers (mm)")
    if ext.size and (ext.min() < 0 or ext.max() > np.iinfo(np.int32).max):
        raise ValueError("extents must lie in [0, 2^31)")
    return np.ascontiguousarray(ext, dtype=np.int32)


def grid_dims_batch(extents, bin=100):
    """grid_dims for every tile: (widths int32 [n_tiles], heights int32 [n_tiles], pixel_offset int64 [n_tiles + 1]);
    tile t's image is pixels pixel_offset[t] .. pixel_offset[t + 1] - 1 of the batch image (bs_grid_dims_batch)."""
    ext = np.asarray(extents)
    if ext.ndim != 2 or len(ext) == 0:
        raise ValueError("extents must be a non-empty [n_tiles, 3] array")
    ext = _tile_extents(ext, len(ext))
    nt = len(ext)
    w = np.empty(nt, dtype=np.int32)
    h = np.empty(nt, dtype=np.int32)
    po = np.empty(nt + 1, dtype=np.int64)
    rc = _lib.load().bs_grid_dims_batch(ext.ctypes.data, nt, int(bin), w.ctypes.data, h.ctypes.data, po.ctypes.data)
    if rc != 0:
        raise ValueError("bs_grid_dims_batch: invalid extent / bin")
    return w, h, po


def grid_dims(extent, bin=100):
    """(width, height) of the 2-D raster (TMC3.cpp:75-76)."""
    ext = np.ascontiguousarray(extent, dtype=np.int32)
    w, h = C.c_int32(0), C.c_int32(0)
    rc = _lib.load().bs_grid_dims(ext.ctypes.data, bin, C.byref(w), C.byref(h))
    if rc != 0:
        raise ValueError("bs_grid_dims: invalid extent / bin")
    return w.value, h.value


def save_image(image, prefix):
    """buildingSeg::save_image (TMC3.cpp:81-117): three 8-bit RGB PNGs -- mean height in the
    red channel, density in the green channel, and the (never written, all zero) third
    channel in green.  Each channel is scaled by its maximum and truncated to uint8.
    The reference's file names are prefix + a Chinese caption; this port uses ASCII
    suffixes (height / density / density_height).  Returns the three uint8 arrays."""
    img = np.asarray(image, dtype=np.float64)
    h, w, _ = img.shape
    mx = [max(0.0, float(img[..., c].max())) for c in range(3)]  # `max` starts at 0 (TMC3.cpp:85)
    outs = []
    for c, slot, name in ((0, 0, "height"), (1, 1, "density"), (2, 1, "density_height")):
        out = np.zeros((h, w, 3), dtype=np.uint8)
        if mx[c] != 0:
            out[..., slot] = (255.0 * (1.0 * img[..., c] / mx[c])).astype(np.uint8)
        write_png(prefix + name + ".png", out)
        outs.append(out)
    return outs


def write_png(path, rgb):
    """Minimal 8-bit RGB PNG writer (zlib from the standard library)."""
    import struct
    import zlib
    rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].tobytes() for y in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


_DEFAULT_CTX = None


def _ctx() -> Context:
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = Context(0)
    return _DEFAULT_CTX


def get_normal_and_k_neighbor(point_cloud, k: int = 15, ctx: Context | None = None):
    """get_Normal_and_K_neighbor<K>(pointCloud, normal, neigh) (my_function.h:48-85).
    Returns (normal [n,3] f64, neigh [n,K] int32).  The reference's stray
    output.ply side effect (my_function.h:81) is not reproduced."""
    neigh, normals = (ctx or _ctx()).knn_normals(point_cloud, default_params(k=k))
    return normals, neigh


class SegPlane:
    """class seg_plane (my_function.h:89-123)."""

    def __init__(self, point_cloud, normal, neigh, num_neigh: int, ctx: Context | None = None):
        self.cloud = np.ascontiguousarray(point_cloud, dtype=np.int32)
        self.normal = np.ascontiguousarray(normal, dtype=np.float64)
        self.neigh = np.ascontiguousarray(neigh, dtype=np.int32)
        self.K = int(num_neigh)
        self.planeIdx = np.full(len(self.cloud), -1, dtype=np.int32)  # my_function.h:103
        self._ctx = ctx or _ctx()

    def get_planes(self):
        """seg_plane::get_planes (my_function.cpp:180-217)."""
        self.planeIdx, planes = self._ctx.region_grow(self.cloud, self.normal, self.neigh,
                                                      default_params(k=self.K))
        return planes

    def set_plane_color(self, planes, rand=None):
        """seg_plane::set_plane_color (my_function.cpp:260-275): colours [n,3]
        uint16 in the reference's G,B,R slots.  ``rand`` is a callable returning
        the next rand() value (default: glibc rand() seeded with 1, as an
        unseeded C program)."""
        if rand is None:
            libc = C.CDLL(None)
            libc.srand(1)
            rand = libc.rand
        colors = np.zeros((len(self.cloud), 3), dtype=np.uint16)
        for p in planes:
            col = [55 + rand() % 200, 55 + rand() % 200, 55 + rand() % 200]
            colors[p.pointIdx] = col
        return colors
