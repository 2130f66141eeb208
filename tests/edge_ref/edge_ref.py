"""Plain numpy restatements, in int64 / float64, of the O(N) device entry points either side of the hot path
(csrc/bs_prepost.hip, bs_grid.hip, bs_shard.hip; include/bs_api.h): PLY ingest, the origin shift and its per-tile form, the
tile boxes, the colour scatter, labels from owners, the row remap and the components of the union-find hook.  One function
per entry point; nothing here knows a tile size, a wave or a launch shape."""
import numpy as np

LO, HI = -2147483649.0, 2147483648.0  # a product is accepted strictly inside (LO, HI)


def field(records, n, stride, offset, is_f64):
    """The scalar at `offset` of each of the n byte-packed records, as float64 (float32 is promoted)."""
    buf = np.frombuffer(bytes(records), np.uint8)
    w = 8 if is_f64 else 4
    idx = np.arange(n, dtype=np.int64)[:, None] * stride + offset + np.arange(w, dtype=np.int64)[None, :]
    return np.ascontiguousarray(buf[idx]).view("<f8" if is_f64 else "<f4").reshape(n).astype(np.float64)


def ingest(records, n, stride, offsets, is_f64, scale):
    """(xyz int32 [n, 3], bad): xyz = trunc(float64(value) * scale) toward zero; bad iff a product is outside (LO, HI) or
    is not a number (such an entry of xyz is left 0: the call fails and the caller must not read it)."""
    xyz = np.zeros((n, 3), np.int32)
    bad = False
    for a, o in enumerate(offsets):
        with np.errstate(over="ignore", invalid="ignore"):
            v = field(records, n, stride, o, is_f64) * np.float64(scale)
        ok = (v > LO) & (v < HI)  # (a NaN compares false)
        bad = bad or not bool(ok.all())
        xyz[ok, a] = np.trunc(v[ok]).astype(np.int64)
    return xyz, bad


def shift(xyz):
    """(xyz - min as int64, min)"""
    x = np.asarray(xyz).astype(np.int64)
    mn = x.min(0)
    return x - mn, mn


def tile_boxes(xyz, off):
    """{min x, y, z, max x, y, z} of every tile [off[t], off[t + 1]): int64 [n_tiles, 6]"""
    x = np.asarray(xyz).astype(np.int64)
    off = np.asarray(off, np.int64)
    return np.array([np.concatenate([x[a:b].min(0), x[a:b].max(0)]) for a, b in zip(off[:-1], off[1:])], np.int64).reshape(-1, 6)


def shift_tiles(xyz, off):
    """(every point minus its own tile's minimum as int64, the minima [n_tiles, 3])"""
    x = np.asarray(xyz).astype(np.int64)
    off = np.asarray(off, np.int64)
    mn = tile_boxes(x, off)[:, :3]
    return x - np.repeat(mn, np.diff(off), axis=0), mn


def colours(n, planes, rgb):
    """uint16 [n, 3]: rgb[i] at every point index of planes[i], 0 elsewhere (planes are disjoint)"""
    out = np.zeros((n, 3), np.uint16)
    rgb = np.asarray(rgb, np.int64).reshape(-1, 3)
    for i, idx in enumerate(planes):
        out[np.asarray(idx, np.int64)] = rgb[i].astype(np.uint16)
    return out


def labels_from_owner(owner, seeds):
    """1 + #(seeds < owner), and -1 for every negative owner"""
    o = np.asarray(owner, np.int64)
    s = np.asarray(seeds, np.int64)
    return np.where(o < 0, -1, np.searchsorted(s, o, "left") + 1).astype(np.int64)


def remap(rows, sorted_gidx):
    """(out, any_missing): the position of every entry of rows in sorted_gidx, 0 where it is missing"""
    r = np.asarray(rows, np.int64)
    g = np.asarray(sorted_gidx, np.int64)
    if len(g) == 0:
        return np.zeros(r.shape, np.int64), bool(r.size)
    pos = np.searchsorted(g, r, "left")
    ok = (pos < len(g)) & (g[np.minimum(pos, len(g) - 1)] == r)
    return np.where(ok, pos, 0).astype(np.int64), bool((~ok).any())


def components(n_total, gidx, rows):
    """parent [n_total]: the smallest id of x's component in the undirected graph with an edge gidx[i] -- rows[i][j] for every
    i, j; a node no edge touches is its own component."""
    import scipy.sparse as sp
    import scipy.sparse.csgraph as cg
    rows = np.asarray(rows, np.int64)
    u = np.repeat(np.asarray(gidx, np.int64), rows.shape[1])
    v = rows.reshape(-1)
    A = sp.coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(n_total, n_total))
    _, lab = cg.connected_components(A, directed=False)
    first = np.full(lab.max() + 1, n_total, np.int64)
    np.minimum.at(first, lab, np.arange(n_total, dtype=np.int64))
    return first[lab]
