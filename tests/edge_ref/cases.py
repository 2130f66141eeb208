"""Inputs of the edge-kernel tests (tests/test_edge_kernels_cpu.py, tests/test_gpu_edge_kernels.py, tests/tools/fuzz_edges.py),
all from fixed seeds, and next to each the boundary it sits on, as integers.

The boundaries (csrc/bs_prepost.hip, bs_grid.hip, bs_shard.hip, bs_common.h):
  WG            256      threads of a workgroup of every kernel here; WAVE 64 lanes
  MINMAX_TRIP   131 072  = 512 workgroups x 256: minmax_kernel's grid-stride loop makes a second trip from n > MINMAX_TRIP
  TILE_CHUNK    4 096    points per block of the segmented bounding-box reduction (tile_bbox_kernel)
  REMAP_TABLE   2^22     entries from which bs_remap_rows_dev takes the look-up table instead of the binary search
  kq            (k+3)>>2 threads per row of cc_hook_kernel
boundaries() lists, per boundary, the case sizes on each side; test_edge_kernels_cpu.py asserts that both sides are there."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


ref = _load("edge_ref", os.path.join(HERE, "edge_ref.py"))

WAVE, WG = 64, 256
MINMAX_TRIP = 512 * WG
TILE_CHUNK = 4096
REMAP_TABLE = 1 << 22
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# ---- PLY fixture values (tests/golden/ply_edge_cases.npz) ------------------------------------------------------------------
PLY_SCALE = 1000.0
PLY_SWEEP = np.arange(-5000, 5001)  # x = k / 1000
# what the sweep holds on the CPU (asserted by test_edge_kernels_cpu.py before a GPU is asked)
SWEEP_F64_TRUNC_NOT_K = 96        # trunc(float64(k / 1000) * 1000) != k
SWEEP_F64_TRUNC_NOT_FLOOR = 82    # ... and truncation differs from floor (the negative non-integers)
SWEEP_F32_TRUNC_NOT_K = 4946      # float32(k / 1000) promoted, then * 1000
SWEEP_F32_PRODUCT_DIFFERS = 4856  # of those, a float32 product would truncate to yet another value


def _largest_fitting(dt, scale, sign):
    """the value of type dt of the largest magnitude whose float64 product with scale is still accepted"""
    v = dt(sign * (2147483648.0 if sign > 0 else 2147483649.0) / scale)
    while not (ref.LO < np.float64(v) * np.float64(scale) < ref.HI):
        v = np.nextafter(v, dt(0))
    return v


def ply_special_values(is_f64):
    """(kind, value) pairs beside the sweep: negative fractions, signed zeros, subnormals, one ulp either side of an integer
    number of millimetres, the largest magnitudes that still fit after scaling"""
    dt = np.float64 if is_f64 else np.float32
    out = [("neg_fraction", dt(v)) for v in (-0.0005, -0.0009999, -0.0010001, -0.0015, -0.9999, -1.9995, -7.0004, -123.4567)]
    out += [("zero", dt(0.0)), ("zero", dt(-0.0))]
    tiny, fi = np.nextafter(dt(0), dt(1)), np.finfo(dt)
    out += [("subnormal", s * v) for s in (dt(1), dt(-1)) for v in (tiny, dt(fi.tiny) - tiny, dt(fi.tiny) / dt(4))]
    for mm in (1, 2, 7, 999, 1000, 1001, 4096, 123456, 2147483):
        for s in (1, -1):
            c = dt(s * mm / 1000.0)
            out += [("ulp_below", np.nextafter(c, dt(-np.inf))), ("ulp_at", c), ("ulp_above", np.nextafter(c, dt(np.inf)))]
    out += [("largest", _largest_fitting(dt, PLY_SCALE, 1)), ("largest", _largest_fitting(dt, PLY_SCALE, -1))]
    return out


def ply_edge_values(is_f64):
    """[n, 3] coordinates of the fixture file: the sweep on x, the special values cycling on y and (from the other end) on z"""
    dt = np.float64 if is_f64 else np.float32
    sp = np.array([v for _, v in ply_special_values(is_f64)], dtype=dt)
    n = len(PLY_SWEEP)
    xyz = np.empty((n, 3), dt)
    xyz[:, 0] = (PLY_SWEEP / 1000.0).astype(dt)
    xyz[:, 1] = sp[np.arange(n) % len(sp)]
    xyz[:, 2] = sp[::-1][(np.arange(n) * 7) % len(sp)]
    return xyz


# the two files: (name, is_f64, properties as (ply type, name, numpy type)); strides 27 and 21, coordinates at odd offsets
PLY_EDGE_FILES = (
    ("edge_f64", True, [("uchar", "red", "u1"), ("float64", "x", "<f8"), ("float64", "y", "<f8"), ("float64", "z", "<f8"),
                        ("uchar", "green", "u1"), ("uchar", "blue", "u1")]),
    ("edge_f32", False, [("uchar", "red", "u1"), ("float", "z", "<f4"), ("float32", "intensity", "<f4"), ("float", "x", "<f4"),
                         ("uint16", "ring", "<u2"), ("float32", "y", "<f4"), ("uchar", "green", "u1"), ("uchar", "blue", "u1")]),
)


def ply_edge_file(name):
    """the bytes of a fixture input file (header + binary little-endian body)"""
    _, is_f64, props = next(f for f in PLY_EDGE_FILES if f[0] == name)
    xyz = ply_edge_values(is_f64)
    n = len(xyz)
    rec = np.zeros(n, dtype=[(p, d) for _, p, d in props])
    for a, p in enumerate("xyz"):
        rec[p] = xyz[:, a]
    for p, d in ((p, d) for _, p, d in props if p not in "xyz"):
        rec[p] = (np.arange(n) * 37 + len(p)) % 251
    hdr = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"] + [f"property {t} {p}" for t, p, _ in props]
    hdr += ["end_header"]
    return ("\n".join(hdr) + "\n").encode() + rec.tobytes()


# ---- synthetic ingest ----------------------------------------------------------------------------------------------------
INGEST_STRIDES = (12, 15, 24, 27, 40)
INGEST_ORDERS = ("xyz", "zxy", "rgb_first")
INGEST_N = (1, 63, 64, 65, 255, 256, 257, 4097)  # either side of a wave, of a workgroup, and 17 workgroups
INGEST_SCALES = (1000.0, 1.0, 0.001, -1000.0)


def ingest_offsets(stride, order, is_f64):
    """byte offsets of (x, y, z), or None where the record has no room for that layout"""
    w = 8 if is_f64 else 4
    if order == "xyz":
        off = (0, w, 2 * w)
    elif order == "zxy":
        off = (w, 2 * w, 0)
    else:
        off = (3, 3 + w, 3 + 2 * w)  # three colour bytes first: odd offsets
    return off if max(off) + w <= stride else None


def ingest_records(rng, n, stride, off, is_f64, scale, extent_limit=True):
    """n byte-packed records with random bytes everywhere but in the coordinates; the products stay within +-1e9 (so that the
    extent stays below 2^31 for the shift) and have fractions of both signs"""
    dt = "<f8" if is_f64 else "<f4"
    w = 8 if is_f64 else 4
    buf = rng.integers(0, 256, n * stride, dtype=np.uint8)
    mag = (1.0e9 if extent_limit else 2.0e9) / abs(scale)
    for o in off:
        v = rng.uniform(-mag, mag, n)
        whole = rng.random(n) < 0.25
        v[whole] = np.round(v[whole])  # some products that are integers already
        v[rng.random(n) < 0.1] /= 1.0e10  # some values near zero: products in (-1, 1) of both signs
        raw = np.ascontiguousarray(v.astype(dt)).view(np.uint8).reshape(n, w)
        idx = np.arange(n)[:, None] * stride + o + np.arange(w)[None, :]
        buf[idx] = raw
    return buf


def ingest_layouts():
    """every (stride, order, is_f64, offsets) of the lists above that fits"""
    return [(s, o, f, ingest_offsets(s, o, f)) for s in INGEST_STRIDES for o in INGEST_ORDERS for f in (False, True)
            if ingest_offsets(s, o, f) is not None]


# the ends of the range at scale 1: (value, type, what it must give)
INGEST_ENDS = (
    (np.nextafter(2147483648.0, 0.0), "<f8", I32_MAX),
    (np.nextafter(-2147483649.0, 0.0), "<f8", I32_MIN),
    (float(np.nextafter(np.float32(2147483648.0), np.float32(0))), "<f4", 2147483520),  # the largest float32 below 2^31
    (-2147483648.0, "<f4", I32_MIN),
    (-2147483648.0, "<f8", I32_MIN),
    (2147483647.0, "<f8", I32_MAX),
)
# rejected at scale 1 (BS_ERR_RANGE).  -2147483649 is no float32: the nearest one below -2^31 takes its place there.
INGEST_REJECTED = {
    "<f8": (2147483648.0, -2147483649.0, float("nan"), float("inf"), float("-inf")),
    "<f4": (2147483648.0, float(np.nextafter(np.float32(-2147483648.0), np.float32(-np.inf))), float("nan"), float("inf"),
            float("-inf")),
}
INGEST_REJECT_N = 300  # two workgroups, the last one partial (44 records)
INGEST_REJECT_AT = ((0, 0), (INGEST_REJECT_N - 1, 1), (137, 2))  # (record, axis): first record; last record of the partial
#                                                                  workgroup; z only


# ---- shift ---------------------------------------------------------------------------------------------------------------
SHIFT_N = (1, 64, MINMAX_TRIP - 1, MINMAX_TRIP, MINMAX_TRIP + 1, 2 * MINMAX_TRIP + 1)
SHIFT_PLACES = ("first", "last", "lanes")


def shift_min_indices(n, place):
    """index of the minimum of x, y, z.  'lanes': a different lane (index % 64) and workgroup for each axis; from
    MINMAX_TRIP + 1 on the first of them (and the third, where n allows) lies where only the second trip of the grid-stride loop
    reads"""
    if place == "first":
        return (0, 0, 0)
    if place == "last":
        return (n - 1, n - 1, n - 1)
    if n > MINMAX_TRIP:
        far = MINMAX_TRIP + 5 * WG + 17
        return (MINMAX_TRIP + (n - 1 - MINMAX_TRIP) // 2, (n - 1) // 3 | 1, far if n > far else (2 * (n - 1)) // 3)
    return ((n - 1) // 2, (n - 1) // 3, (2 * (n - 1)) // 3 + (1 if n > 3 else 0))


def shift_cloud(n, place, seed=0):
    rng = np.random.default_rng([n, SHIFT_PLACES.index(place), seed])
    xyz = rng.integers(-1000, 1000, (n, 3), dtype=np.int64) + np.array([5000, -250, 77])
    for a, i in enumerate(shift_min_indices(n, place)):
        xyz[i, a] = xyz[:, a].min() - 1 - a
    return xyz.astype(np.int32)


def shift_further_clouds():
    """(name, cloud): all points equal; negative coordinates; minimum -2^31 with the largest extent of the contract, 2^31 - 1"""
    rng = np.random.default_rng(77)
    wide = rng.integers(I32_MIN, 0, (1000, 3), dtype=np.int64)
    wide[3], wide[998] = I32_MIN, -1
    return [("equal", np.full((300, 3), -123456, np.int32)),
            ("negative", rng.integers(-2_000_000_000, -1_000_000_000, (1000, 3), dtype=np.int64).astype(np.int32)),
            ("widest", wide.astype(np.int32))]


# ---- tiles ---------------------------------------------------------------------------------------------------------------
TILE_BATCHES = {
    "mixed": (1, TILE_CHUNK - 1, TILE_CHUNK, TILE_CHUNK + 1, 2 * TILE_CHUNK + 1, 1, 1, 3 * TILE_CHUNK + 1),
    "thousand_points": (1,) * 1000,
    "one_tile": (5000,),
}


def tile_extreme_places(length):
    """where a tile's extreme values sit: the first point, the last one, and either side of the first chunk boundary"""
    return sorted({0, length - 1, min(TILE_CHUNK - 1, length - 1), min(TILE_CHUNK, length - 1)})


def tile_batch(name, seed=0):
    """(xyz int32 [n, 3], off int64 [n_tiles + 1]); of tile t the minimum of axis a sits at place (a + t) and the maximum at
    place (a + t + 1), counted round the places of tile_extreme_places"""
    lens = TILE_BATCHES[name]
    rng = np.random.default_rng([sorted(TILE_BATCHES).index(name), seed])
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    xyz = rng.integers(-1000, 1000, (off[-1], 3), dtype=np.int64)
    for t, ln in enumerate(lens):
        xyz[off[t]:off[t + 1]] += rng.integers(-1_000_000, 1_000_000, 3)
        pl = tile_extreme_places(ln)
        for a in range(3 if ln > 1 else 0):
            xyz[off[t] + pl[(a + t) % len(pl)], a] -= 5000 + a
            xyz[off[t] + pl[(a + t + 1) % len(pl)], a] += 5000 + a
    return xyz.astype(np.int32), off


# ---- colours -------------------------------------------------------------------------------------------------------------
COLOUR_CLOUDS = ("plane_cube_12k", "walls_6k", "facade_10k_k16")  # tests/golden: at most 12 000 points
COLOUR_BIG_PLANE = TILE_CHUNK  # a plane of more points than 16 x 256 makes color_scatter_kernel's loop take a second trip


def colour_table(n_planes, seed=0):
    """colour values over the whole of 0 .. 65535, the two ends included"""
    rgb = np.random.default_rng([n_planes, seed]).integers(0, 65536, (n_planes, 3))
    if n_planes:
        rgb[0] = (65535, 0, 1)
    return rgb.astype(np.int32)


def no_plane_cloud(n=600, seed=5):
    """points scattered so thinly that no plane commits"""
    return np.random.default_rng(seed).integers(0, 4_000_000, (n, 3)).astype(np.int32)


# ---- labels from owners ----------------------------------------------------------------------------------------------------
LABEL_N_SEEDS = (0, 1, 2, 1000, 100_000)
LABEL_SMALL_N = (0, 255, 256, 257)


def label_case(n_seeds, n=None, seed=0):
    """(owner, seeds, kinds): owners of every kind -- -1, -2, every seed, strictly between two seeds, below the first seed, above
    the last -- shuffled; kinds[i] names the kind of owner[i]"""
    rng = np.random.default_rng([n_seeds, seed])
    seeds = np.sort(rng.choice(np.arange(10, 10 + 4 * max(n_seeds, 1)), n_seeds, replace=False)).astype(np.int64)
    own, kind = [-1, -2, I32_MIN], ["minus1", "minus2", "negative"]
    own += seeds.tolist()
    kind += ["seed"] * n_seeds
    if n_seeds:
        gaps = np.flatnonzero(np.diff(seeds) > 1)
        own += (seeds[gaps] + 1).tolist() + [0, int(seeds[0]) - 1, int(seeds[-1]) + 1, int(seeds[-1]) + 1000, I32_MAX]
        kind += ["between"] * len(gaps) + ["below", "below", "above", "above", "above"]
    else:
        own += [0, 5, I32_MAX]
        kind += ["no_seeds"] * 3
    own, kind = np.array(own, np.int64), np.array(kind)
    if n is not None:
        pick = rng.integers(0, len(own), n)
        own, kind = own[pick], kind[pick]
    p = rng.permutation(len(own))
    return own[p].astype(np.int32), seeds.astype(np.int32), kind[p]


# ---- remap -----------------------------------------------------------------------------------------------------------------
REMAP_K = (1, 3, 16)
# rows x k either side of REMAP_TABLE: exactly 2^22 - 1 and 2^22 where k divides them (2^22 - 1 = 3 x 1 398 101), the nearest
# multiple of k otherwise.  The cap of 2^20 workgroups (2^28 entries, 1 GiB of rows) is not reachable at test size.
REMAP_ROWS = {1: (REMAP_TABLE - 1, REMAP_TABLE), 3: ((REMAP_TABLE - 1) // 3, (REMAP_TABLE + 2) // 3), 16: (REMAP_TABLE // 16 - 1, REMAP_TABLE // 16)}
REMAP_LOCAL, REMAP_SPAN = 300_000, 3 << 20  # sorted_gidx: 300 000 of the ids below 3 x 2^20 (its last entry stays below 2^24)


def remap_input(seed=0):
    """(flat, sorted_gidx): REMAP_TABLE + 2 entries, all present, to be cut into rows of every k"""
    rng = np.random.default_rng([9, seed])
    sg = np.sort(rng.choice(REMAP_SPAN, REMAP_LOCAL, replace=False)).astype(np.int32)
    flat = sg[rng.integers(0, len(sg), REMAP_TABLE + 2)]
    flat[:4] = (sg[0], sg[-1], sg[0], sg[-1])
    return flat, sg


def remap_missing(sg):
    """{kind: values that are not in sg}"""
    inside = int(np.setdiff1d(np.arange(int(sg[0]), int(sg[-1])), sg)[len(sg) // 2])
    return {"negative": (-1, -5, I32_MIN), "last_plus_1": (int(sg[-1]) + 1,), "far_above": ((1 << 24) + 5, I32_MAX),
            "inside_absent": (inside,)}


# ---- hooking ---------------------------------------------------------------------------------------------------------------
HOOK_K = (1, 2, 3, 4, 5, 7, 8, 15, 16, 63, 64)  # kq = 1, 1, 1, 1, 2, 2, 2, 4, 4, 16, 16; k = 4, 8, 16, 64 fill the last quad
HOOK_N_TOTAL = 20_000


def hook_case(k, permuted, seed=0, n_total=HOOK_N_TOTAL):
    """(gidx int32 [m], rows int32 [m, k]): gidx a random third of the ids, sorted or permuted; rows random ids in [0, n_total)
    with self loops, repeated entries, and a slot 0 that is the point itself in every fourth row only"""
    rng = np.random.default_rng([k, int(permuted), seed])
    m = n_total // 3
    gidx = np.sort(rng.choice(n_total, m, replace=False))
    if permuted:
        gidx = rng.permutation(gidx)
    # few distinct targets per row keep the graph in many components of every size for every k
    near = rng.integers(0, n_total, (m, 2))
    rows = near[np.arange(m)[:, None], rng.integers(0, 2, (m, k))]
    rows[::4, 0] = gidx[::4]  # slot 0 = the point itself
    if k > 1:
        rows[1::5, k - 1] = gidx[1::5]  # a self loop in the last slot (the one `j < k` guards)
        rows[2::7, k - 1] = rng.integers(0, n_total, len(rows[2::7]))  # an edge only the last slot carries
    return gidx.astype(np.int32), rows.astype(np.int32)


HOOK_RANKS = (2, 3)
HOOK_GRAPHS = ("path", "two_paths")


def hook_graph(name, seed=0):
    """(n_total, order, rows [n, 2]) of a graph of at most 2 048 nodes that needs several hook / MIN rounds: order[i] is the id
    of the i-th node along the walk, rows[i] = (its own id, the next node's id).  'path': one path of 2 048 nodes with permuted
    ids; 'two_paths': two paths of 1 024 nodes joined at their far ends."""
    rng = np.random.default_rng([3, HOOK_GRAPHS.index(name), seed])
    n = 2048
    order = rng.permutation(n)
    nxt = np.roll(order, -1)
    nxt[-1] = order[-1]  # the last node has a self loop
    if name == "two_paths":
        # walk 0 .. 1023 and 1024 .. 2047 start at their own ends; the far ends (1023 and 2047) are joined
        nxt[1023] = order[2047]
    return n, order.astype(np.int32), np.stack([order, nxt], axis=1).astype(np.int32)


def hook_deal(order, rows, ranks):
    """the walk's i-th node goes to rank i mod ranks: [(gidx, rows)] per rank"""
    return [(np.ascontiguousarray(order[r::ranks]), np.ascontiguousarray(rows[r::ranks])) for r in range(ranks)]


def hook_rounds(n_total, deal, hook, cap=None):
    """The protocol of include/bs_api.h: every round a hook per rank on that rank's parent array, then the elementwise minimum
    handed to every rank; until no rank hooks.  hook(rows, gidx, parent) -> hooks (parent updated in place).  Returns
    (parent, rounds, hooks per round); rounds counts the final round without hooks."""
    cap = n_total if cap is None else cap
    parents = [np.arange(n_total, dtype=np.int32) for _ in deal]
    per_round = []
    while len(per_round) < cap:
        h = [hook(rows, gidx, p) for (gidx, rows), p in zip(deal, parents)]
        mn = np.minimum.reduce(parents)
        parents = [mn.copy() for _ in deal]
        per_round.append(sum(h))
        if not any(h):
            break
    return parents[0], len(per_round), per_round


# ---- fuzz ------------------------------------------------------------------------------------------------------------------
FUZZ_ENTRIES = ("ingest", "shift", "tiles", "labels", "remap", "hook")
FUZZ_CASES = 40


def _around(rng, points, spread=3):
    return int(max(1, rng.choice(points) + rng.integers(-spread, spread + 1)))


def fuzz_case(entry, seed):
    """one seeded input of `entry`, with sizes and layouts drawn around the boundaries above: a dict the runner of
    tests/tools/fuzz_edges.py understands"""
    rng = np.random.default_rng([FUZZ_ENTRIES.index(entry), seed])
    if entry == "ingest":
        s, o, f, off = ingest_layouts()[rng.integers(0, len(ingest_layouts()))]
        n = _around(rng, (1, WAVE, WG, 2 * WG, 4097))
        scale = float(rng.choice(INGEST_SCALES + (0.5, -1.0, 1.0e-6)))
        return dict(n=n, stride=s, order=o, is_f64=f, off=off, scale=scale, shift=bool(rng.integers(0, 2)),
                    lead=int(rng.integers(0, 8)), records=ingest_records(rng, n, s, off, f, scale))
    if entry == "shift":
        n = _around(rng, (1, WAVE, WG, MINMAX_TRIP, MINMAX_TRIP, 2 * MINMAX_TRIP))
        lo = int(rng.choice((I32_MIN, -1_000_000, 0, 1_000_000_000)))
        ext = int(rng.choice((1, 1000, I32_MAX)))
        xyz = rng.integers(lo, min(lo + ext, I32_MAX), (n, 3), dtype=np.int64, endpoint=True)
        for a in range(3):
            xyz[rng.integers(0, n), a] = lo
        return dict(n=n, xyz=xyz.astype(np.int32))
    if entry == "tiles":
        nt = int(rng.choice((1, 2, 7, 300)))
        lens = [_around(rng, (1, 1, TILE_CHUNK, TILE_CHUNK, 2 * TILE_CHUNK) if nt < 300 else (1, 1, 2, 5), 2) for _ in range(nt)]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        xyz = rng.integers(-1_000_000_000, 1_000_000_000, (off[-1], 3), dtype=np.int64)
        return dict(n=int(off[-1]), off=off, xyz=xyz.astype(np.int32))
    if entry == "labels":
        ns = int(rng.choice((0, 1, 2, 3, 255, 256, 257, 1000)))
        own, seeds, kinds = label_case(ns, n=_around(rng, (1, WG, 2 * WG, 5000)), seed=seed + 1)
        return dict(owner=own, seeds=seeds, kinds=kinds)
    if entry == "remap":
        k = int(rng.choice((1, 2, 3, 15, 16)))
        n_loc = _around(rng, (1, 2, WG, 5000))
        sg = np.sort(rng.choice(4 * n_loc + 8, n_loc, replace=False)).astype(np.int32)
        rows = rng.integers(-2, int(sg[-1]) + 3, (_around(rng, (1, WG, 1000)), k)).astype(np.int32)
        return dict(rows=rows, sg=sg)
    if entry == "hook":
        k = int(rng.choice(HOOK_K))
        n_total = _around(rng, (2, WG, 3000), 1) + 1
        m = int(rng.integers(1, n_total + 1))
        gidx = rng.permutation(n_total)[:m]
        if rng.integers(0, 2):
            gidx = np.sort(gidx)
        pool = rng.integers(0, n_total, (m, 2))
        rows = pool[np.arange(m)[:, None], rng.integers(0, 2, (m, k))]
        return dict(n_total=n_total, k=k, gidx=gidx.astype(np.int32), rows=rows.astype(np.int32))
    raise ValueError(entry)


# ---- reach -----------------------------------------------------------------------------------------------------------------
def boundaries():
    """{boundary: (its value, the case sizes below it or at its low side, the case sizes at or above its high side)} from the
    case lists of this file alone"""
    def sides(b, sizes, at_is_low=False):
        lo = [s for s in sizes if (s <= b if at_is_low else s < b)]
        hi = [s for s in sizes if (s > b if at_is_low else s >= b)]
        return b, lo, hi
    mixed = TILE_BATCHES["mixed"]
    out = {
        "ingest: records of a wave (64)": sides(WAVE, INGEST_N, True),
        "ingest: records of a workgroup (256)": sides(WG, INGEST_N, True),
        "ingest: product below 2^31": (1 << 31, [int(v) for v, _, w in INGEST_ENDS if w > 0], [int(v) for v in INGEST_REJECTED["<f8"][:1]]),
        "ingest: product above -2^31 - 1": (-(1 << 31) - 1, [int(v) for v in INGEST_REJECTED["<f8"][1:2]], [int(np.ceil(v)) for v, _, w in INGEST_ENDS if w < 0]),
        "shift: points of one grid-stride trip (131072)": sides(MINMAX_TRIP, SHIFT_N, True),
        "tiles: points of a chunk (4096)": sides(TILE_CHUNK, mixed, True),
        "tiles: points of two chunks (8192)": sides(2 * TILE_CHUNK, mixed, True),
        "tiles: points of three chunks (12288)": sides(3 * TILE_CHUNK, mixed, True),
        "tiles: one tile / many": sides(2, [len(v) for v in TILE_BATCHES.values()]),
        "labels: no seeds / seeds": sides(1, LABEL_N_SEEDS),
        "labels: owners of a workgroup (256)": sides(WG, LABEL_SMALL_N, True),
        "remap: entries of the table path (2^22)": sides(REMAP_TABLE, [r * k for k in REMAP_K for r in REMAP_ROWS[k]]),
    }
    for q in (1, 2, 4):
        out[f"hook: k fills {q} quad(s) ({4 * q})"] = sides(4 * q, HOOK_K, True)
    out["hook: the largest k (64)"] = sides(64, HOOK_K)
    return out
