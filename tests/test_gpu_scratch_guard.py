"""Every stage's scratch under guard: overruns past what a stage requested, and reads of scratch nothing wrote.

All device memory of a context comes from DevBuf::reserve (csrc/bs_common.h), which normally hands out 12.5 % + 256 B
more than a stage asks for, only ever grows, and never looks at what hipMalloc returned; the stages cut their buffers
into sub-arrays by hand.  bs_selftest_scratch_guard (include/bs_api.h) makes a context allocate exactly what is
requested plus a guard filled with a canary, and fill the requested bytes with a poison byte; bs_selftest_scratch_check
reads the guards back and names the damaged buffers by their bs_ctx member (`rf[9]`).  This module runs the smallest
named cases of every stage -- through the check helpers of the stage's own GPU module, so against the same exact
references, every comparison == -- on FRESH guarded contexts:

  canary   canary only, a fresh context per CASE: the results equal the references and no guard is damaged (on a
           shared context a smaller case after a larger one would take the early return of reserve and its overrun
           would land inside the larger request);
  poison   canary + poison: POISON[0] on a fresh context per case, POISON[1] on one context for the whole stage (the
           cases also meet what earlier cases left); the same, and every returned array and figure is byte-identical
           between the two (timings and the ms_* fields apart);
  order    for the stages that keep no state between calls and for the count/emit chains: on one poisoned context a
           larger case A, a smaller case B, A again, and on another B, A, B -- equal to the references every time;
  limits   the capacity limits of tests/test_gpu_grow_limits.py that fill the grower's hand-sized pools to the brim;
  coverage every member group of bs_ctx (each array, each single buffer) was allocated under guard and checked by some
           test of this module: test_every_member_group_was_allocated_under_guard, which runs last.

Cases are chosen by four rules: the smallest non-empty case and the empty one; sizes one below and one above a multiple
of 64 and of 256 items, 31/32/33 wide images for the tiled image stages, and for the 64 x 16 labelling tile of
bs_building.hip over the padded image 61/62/63 wide and 13/14/15 high; the case that takes each non-default memory path
where a small one exists; named cases only (no fuzz seeds, no full-size images).

How to run one stage under the guard: `pytest tests/test_gpu_scratch_guard.py -k roofs`; from Python,
`ctx = api.Context(0); ctx.selftest_scratch_guard(canary=True, poison=0x5D)` right after the context is made, then any
call, then `ctx.selftest_scratch_check()`.

Wall time on the MI355X: 28 s for the whole file, 85 tests (the 12 limit scenarios, three grows each, take 19 s of it);
tests/test_gpu_grow_limits.py takes 75 s in the same run on the same machine.  Nothing had to be cut.

Findings so far ("Guarded scratch"): the round pool's never-written words read by reset_tags_kernel after a
pool exhaustion (test_limits[v2-facade400_k16-pool_cap] faulted under the poison before the fix); no damaged canary."""
import dataclasses
import os
import struct
import sys

import numpy as np
import pytest

from buildingsegment_amd import _lib, api, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
for _d in ("footprint_ref", "building_ref", "shard_ref"):  # (as the stage modules do for their references)
    if os.path.join(HERE, _d) not in sys.path:
        sys.path.insert(0, os.path.join(HERE, _d))

# Neither 0x00 nor 0xFF.  As int32 0x5D5D5D5D = 1 566 399 837 is above every index, label and count of a test-size case and
# is none of the sentinels (-1, -2, INT32_MAX, INT32_MIN, EMPTY); 0xA6A6A6A6 = -1 499 027 802 is negative and none of them
# either.  As f64 they read 6.5e141 and -1.2e-120: no coordinate, normal component or height.
POISON = (0x5D, 0xA6)
assert all(p not in (0x00, 0xFF) for p in POISON) and POISON[0] != POISON[1]

_ALLOCATED = {}  # bs_ctx member group -> slots of it allocated under guard and checked clean, over the whole module


# ---- contexts, the check, digests --------------------------------------------------------------------------------------
class guarded:
    """a fresh context with the guard set; leaving the block reads every guard back and requires all of them whole"""

    def __init__(self, poison=None):
        self.poison = poison

    def __enter__(self):
        _torch_first()
        self.ctx = api.Context(0)
        self.ctx.selftest_scratch_guard(canary=True, poison=self.poison)
        self.ctx._scratch_poison = self.poison  # (the sharded cases guard their second rank's context the same way)
        return self.ctx

    def __exit__(self, et, ev, tb):
        try:
            if et is None:
                clean(self.ctx)
        finally:
            self.ctx.close()
        return False


def _torch_first():
    # torch must initialise the GPU before the library is loaded (tests/conftest.py, gpu_ctx); this module makes its own
    # contexts and does not use that fixture
    import torch
    if torch.cuda.is_available():
        torch.zeros(1, device="cuda")


def describe(rep):
    return "; ".join(f"{d['name']}: requested {d['requested']} B, damaged +{d['first_bad']} .. +{d['last_bad']} past the request"
                     for d in rep["damaged"])


def clean(ctx):
    """no guard of the context is damaged; records what was allocated for the coverage assertion"""
    rep = ctx.selftest_scratch_check()
    assert rep["n_damaged"] == 0, f"{rep['n_damaged']} scratch buffers overrun: {describe(rep)}"
    slots = ctx.selftest_scratch_list()
    assert rep["n_guarded"] == len(slots) and rep["bytes_requested"] == sum(s["requested"] for s in slots)
    for s in slots:
        group, _, idx = s["name"].partition("[")
        _ALLOCATED.setdefault(group, set()).add(int(idx[:-1]) if idx else 0)
    return rep


def digest(x, out=None, path=""):
    """every array and scalar figure under x as (path, bytes), the ms_* fields (timings) apart.  Nothing else is excluded:
    attributes that begin with an underscore would be handles of the binding, not results, and no result class has one"""
    out = [] if out is None else out
    if isinstance(x, np.ndarray):
        out.append((path, x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes()))
    elif isinstance(x, (bool, int, str, bytes, np.integer, np.bool_)) or x is None:
        out.append((path, repr(x)))
    elif isinstance(x, (float, np.floating)):
        out.append((path, struct.pack("<d", float(x))))
    elif isinstance(x, dict):
        for k in sorted(x):
            if not str(k).startswith("ms_"):
                digest(x[k], out, f"{path}.{k}")
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            digest(v, out, f"{path}[{i}]")
    elif dataclasses.is_dataclass(x) or hasattr(x, "__dict__"):
        for k, v in sorted(vars(x).items()):
            if not k.startswith(("ms_", "_")):
                digest(v, out, f"{path}.{k}")
    else:
        raise TypeError(f"digest: {path} is a {type(x).__name__}")
    return out


def first_difference(a, b):
    da, db = digest(a), digest(b)
    if len(da) != len(db):
        return "the results have different shapes"
    return next((x[0] for x, y in zip(da, db) if x != y), None)


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


class env:
    """an environment switch the library reads on every call, for one block"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


# ---- the stages: name -> [(case id, run(ctx, oracle) -> results)] ------------------------------------------------------
# A run goes through the check helper of the stage's own module, so it asserts equality with the stage's reference; what
# it returns is compared between the two poison runs.  ORDER[stage] = (A, B): a larger and a smaller case id.
STAGES, ORDER = {}, {}


def stage(name, order=None):
    def deco(f):
        STAGES[name] = f
        if order:
            ORDER[name] = order
        return f
    return deco


def _gold(name):
    return np.load(os.path.join(GOLD, name + ".npz"))


@stage("knn", order=("k16_4097", "k15_255"))
def _knn():
    from test_gpu_parity import _check_knn_normals
    import test_gpu_normals as N
    out = []
    for k, n in ((15, 255), (16, 257), (32, 4097), (16, 4097), (16, 16)):  # (n == k: the smallest cloud there is)
        out.append((f"k{k}_{n}", lambda c, O, k=k, n=n: _check_knn_normals(c, O, synth.uniform(n, seed=n + k), k)))
    # r = 181 mm takes the 32-bit relative instance, 182 mm the 64-bit one (tests/test_gpu_normals.py)
    for r in (181, 182):
        out.append((f"radius_{r}", lambda c, O, r=r: _check_knn_normals(c, O, N.cases.committed_cloud("near")[0], 3, radius=float(r),
                                                                       max_nn=64)))
    g = np.arange(24)
    lat = (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * 20).astype(np.int32)
    out.append(("lattice_20mm_all_listed", lambda c, O: _listed(c, _check_knn_normals(c, O, lat, 16), len(lat))))
    far = np.concatenate([synth.uniform(4000, seed=4), np.array([[200000, 5, 5], [5, 300000, 7], [400000, 400000, 400000],
                                                                  [-90000, 0, 0]], np.int32)]).astype(np.int32)
    out.append(("sparse_outliers_far_rings", lambda c, O: _check_knn_normals(c, O, far, 15)))
    out.append(("halo", _halo))
    return out


def _listed(ctx, res, n):
    assert ctx.timings()["n_fallback_queries"] == n
    return res


def _halo(ctx, O):
    """bs_knn_normals_halo as tests/test_gpu_normals.py::test_halo_slabs runs it: the 'near' cloud cut in two"""
    import test_gpu_normals as N
    cases = N.cases
    xyz, cid, sizes = cases.committed_cloud("near")
    p = N._params()
    oneigh, onormals = N._oracle(O, "near", xyz, p)
    cut = 4 * cases.PITCH + cases.BOX + 200
    out = []
    for own, halo in ((xyz[:, 0] < cut, (xyz[:, 0] >= cut) & (xyz[:, 0] < cut + 600)),
                      (xyz[:, 0] >= cut, (xyz[:, 0] < cut) & (xyz[:, 0] >= cut - 600))):
        own_idx, halo_idx = np.nonzero(own)[0].astype(np.int32), np.nonzero(halo)[0].astype(np.int32)
        gidx = np.concatenate([own_idx, halo_idx])
        neigh, normals, unc = ctx.knn_normals_halo(xyz[gidx], gidx, len(own_idx), p, 300.0)
        assert unc == 0 and np.array_equal(neigh, oneigh[own_idx])
        assert np.array_equal(normals.view(np.int64), onormals[own_idx].view(np.int64))
        out.append((neigh, normals))
    return out


def _oracle_segment(O, xyz, k):
    neigh, normals = O.knn_normals(xyz, k=k)
    return (neigh, normals) + tuple(O.region_grow(xyz, normals, neigh))


def _segment(ctx, O, xyz, k, key):
    p = api.default_params(k=k)
    neigh, normals, pi, planes = ctx.segment(xyz, p)
    oneigh, onormals, opi, opl = memo(("segment", key, k), lambda: _oracle_segment(O, xyz, k))
    assert np.array_equal(neigh, oneigh) and np.array_equal(normals, onormals) and np.array_equal(pi, opi)
    assert [q.id for q in planes] == opl["id"].tolist()
    for i, q in enumerate(planes):
        assert np.array_equal(q.pointIdx, opl["point_idx"][opl["offset"][i]:opl["offset"][i + 1]])
        assert np.array_equal(q.center, opl["center"][i]) and np.array_equal(q.normal, opl["normal"][i])
    return neigh, normals, pi, planes


@stage("segment", order=("plane_cube_12k_k15", "walls_6k_k16"))
def _seg():
    from test_gpu_parity import _check_golden
    out = []
    for name, k in (("plane_cube_12k", 15), ("walls_6k", 16), ("plane_cube_12k", 32)):
        out.append((f"{name}_k{k}", lambda c, O, name=name, k=k: _segment(c, O, _gold(name)["xyz"], k, name)))
    out.append(("uniform_16_k16", lambda c, O: _segment(c, O, synth.uniform(16, seed=8), 16, "u16")))  # (nothing grows)
    # region_grow on the reference's own stage-3 fixtures: the sequential grower, the default engine, the first engine
    for name in ("walls_6k", "orphans_p5"):
        path = os.path.join(GOLD, name + ".npz")
        out.append((f"grow_{name}_rg1", lambda c, O, path=path: _check_golden(c, path, 1)))
        out.append((f"grow_{name}_rg0", lambda c, O, path=path: _check_golden(c, path, 0)))
        out.append((f"grow_{name}_first_engine", lambda c, O, path=path: _first_engine(c, path)))
    return out


def _first_engine(ctx, path):
    from test_gpu_parity import _check_golden
    with env(BS_GROW_V2="0"):
        return _check_golden(ctx, path, 2)


@stage("segment_batch", order=("three_tiles_k15", "one_small_tile"))
def _batch():
    from test_gpu_batch import _oracle, _same

    def run(tiles, k, mode, key):
        def f(ctx, O):
            p = api.default_params(k=k, rg_mode=mode)
            want = memo(("batch", key, k), lambda: [_oracle(O, x, p) for x in tiles])
            out = ctx.segment_batch(tiles, p)
            for t, (res, w) in enumerate(zip(out, want)):
                _same(res, w, f"tile {t}")
            return out
        return f

    rng = np.random.default_rng(40)
    small = rng.integers(0, 600, (40, 3)).astype(np.int32)  # a 40-point tile between large ones
    tiles = [_gold("walls_6k")["xyz"], small, synth.uniform(4097, seed=3)]
    return [("three_tiles_k15", run(tiles, 15, 0, "t3")), ("three_tiles_k32_rg1", run(tiles, 32, 1, "t3")),
            ("one_small_tile", run([small], 15, 0, "t1"))]


@stage("ingest_shift_colours", order=("bin_half_mm_300", "bin_f32_random_200"))
def _ingest():
    from test_gpu_ingest import GOLD as PLY, parse_binary

    def ingest(case):
        def f(ctx, O):
            import torch
            buf = PLY[case + "/in"].tobytes()
            n, stride, pos, kind, end = parse_binary(buf)
            want = PLY[case + "/xyz"]
            body = torch.frombuffer(bytearray(buf[end:end + n * stride]), dtype=torch.uint8).cuda()
            d_xyz = torch.empty((n, 3), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            mn = ctx.ingest_dev(body.data_ptr(), n, stride, (pos["x"], pos["y"], pos["z"]), kind["x"] == "float64", d_xyz.data_ptr(),
                                scale=1000.0, shift_to_origin=True)
            got = d_xyz.cpu().numpy()
            assert np.array_equal(mn, want.min(0)) and np.array_equal(got, want - want.min(0))
            return mn, got
        return f

    def shift_and_colours(ctx, O):
        import torch
        raw = _gold("walls_6k")["xyz"].astype(np.int64) + np.array([5000, -250, 77])
        n = len(raw)
        d_xyz = torch.from_numpy(raw.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        mn = ctx.shift_to_origin_dev(d_xyz.data_ptr(), n)
        shifted = (raw - raw.min(0)).astype(np.int32)
        assert mn.tolist() == raw.min(0).tolist() and np.array_equal(d_xyz.cpu().numpy(), shifted)
        d_plane = torch.empty(n, dtype=torch.int32, device="cuda")
        ctx.segment_dev(d_xyz.data_ptr(), n, d_plane.data_ptr(), api.default_params(k=16))
        planes = ctx.planes_fetch()
        opi = memo("walls_shifted", lambda: _oracle_segment(O, shifted, 16)[2])
        assert np.array_equal(d_plane.cpu().numpy(), opi) and len(planes) > 0
        rgb = np.arange(3 * len(planes), dtype=np.int32).reshape(-1, 3) + 60
        d_col = torch.full((n, 3), 999, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        ctx.plane_colors_dev(rgb, n, d_col.data_ptr())
        want = np.zeros((n, 3), np.uint16)
        for i, q in enumerate(planes):
            want[q.pointIdx] = rgb[i]
        got = d_col.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want)
        return mn, got

    return [(c, ingest(c)) for c in ("bin_half_mm_300", "bin_f32_random_200", "bin_f64_nocolor")] + [("shift_and_colours", shift_and_colours)]


def _raster_clouds():
    from test_gpu_fuzz_stages import _tall_cloud
    rng = np.random.default_rng(77)
    out = {n: np.ascontiguousarray(rng.integers(0, 3000, (n, 3)).astype(np.int32)) for n in (255, 257, 4097)}
    out[1] = np.array([[0, 0, 0]], np.int32)
    out["tall"] = _tall_cloud()  # height bins beyond the LDS histogram
    return out


@stage("raster", order=(4097, 255))
def _raster():
    clouds = memo("raster_clouds", _raster_clouds)

    def solo(key):
        def f(ctx, O):
            oimg, oth = memo(("raster", key), lambda: O.grid_picture(clouds[key]))
            img, th = ctx.grid_picture(clouds[key])
            assert th == oth and np.array_equal(img, oimg)
            return img, th
        return f

    def batch(ctx, O):
        keys = (4097, 1, "tall", 255, 257)
        res = ctx.grid_picture_batch([clouds[k] for k in keys])
        for k, (img, th) in zip(keys, res):
            oimg, oth = memo(("raster", k), lambda: O.grid_picture(clouds[k]))
            assert th == oth and np.array_equal(img, oimg), k
        return res

    return [(k, solo(k)) for k in (1, 255, 257, 4097, "tall")] + [("batch", batch)]


def _masks():
    from test_gpu_footprints import SHAPES
    rng = np.random.default_rng(6)
    # 31 / 32 / 33 wide; the labelling tile of bs_building.hip is 64 x 16 over the image padded by one pixel all round, so
    # the sizes that straddle it are 61 / 62 / 63 wide and 13 / 14 / 15 high (padded: 63 / 64 / 65 and 15 / 16 / 17)
    sizes = ((1, 1), (1, 300), (300, 1), (33, 31), (33, 32), (33, 33), (13, 61), (14, 62), (15, 63), (14, 63), (15, 62), (17, 65),
             (63, 63), (65, 65), (33, 129))
    out = {f"{h}x{w}": rng.random((h, w)) < 0.3 for h, w in sizes}
    out["empty"] = np.zeros((7, 7), bool)
    out["rings"] = SHAPES["rings"]
    return out


@stage("footprints", order=("33x129", "15x63"))
def _footprints():
    import ref
    from test_gpu_evidence import eref, same_footprints
    from test_gpu_footprints import _check_image
    from test_gpu_footprints_batch import _check_batch
    masks = memo("masks", _masks)
    out = [(k, lambda c, O, k=k: _check_image(c, ref.image_of_mask(masks[k]))) for k in masks]
    out.append(("batch", lambda c, O: _check_batch(c, [ref.image_of_mask(masks[k]) for k in ("65x65", "empty", "1x300", "rings", "15x63")])))

    def screened(ctx, O):  # with the screen (bs_set_footprint_screen, the host form: fs_dev)
        rng = np.random.default_rng(5)
        img = ref.image_of_mask(masks["33x129"])
        keep = (rng.random((33, 129)) < 0.8).astype(np.uint8)
        ctx.set_footprint_screen(keep)
        try:
            got = ctx.footprints(img, return_mask=True)
        finally:
            ctx.set_footprint_screen(None)
        want, want_mask = eref.screened_footprints(img, keep)
        same_footprints(*got, want, want_mask)
        return got

    return out + [("screened", screened)]


@stage("buildings", order=("65x65", "15x63"))
def _buildings():
    import building_ref as bref
    from test_gpu_buildings import _check_mask, _same_points, _same_votes
    masks = memo("masks", _masks)
    out = [(k, lambda c, O, k=k: _check_mask(c, masks[k])) for k in masks if k != "empty"]
    out.append(("empty", lambda c, O: c.building_map(np.zeros((7, 7), np.uint8))))

    def assign_and_votes(n):
        def f(ctx, O):
            rng = np.random.default_rng(n)
            m = np.zeros((40, 60), np.uint8)
            m[5:15, 5:25] = m[20:35, 30:55] = m[25:30, 2:9] = 1
            bmap, b = ctx.building_map(m * 255)
            r = bref.building_map(m)
            assert np.array_equal(bmap, r.map)
            xyz = np.ascontiguousarray(np.concatenate([rng.integers(0, [6000, 4000], (n, 2)), rng.integers(0, 3000, (n, 1))], 1).astype(np.int32))
            plane = rng.integers(-1, 7, n).astype(np.int32)
            bidx = ctx.assign_buildings(xyz, bmap, b, bin=100, ground_th=1000.0)
            a = bref.assign(xyz, r.map, r.n_buildings, 100, 1000.0)
            _same_points(bidx, b, a)
            v = ctx.plane_buildings(plane, bidx, 5, r.n_buildings)
            _same_votes(v, bref.votes(plane, a.building_idx, 5, r.n_buildings))
            return bidx, b, v
        return f

    def votes_sorted_keys(ctx, O):
        """a vote table of more than 2^22 cells: sorted keys and run lengths in place of the dense histogram (the votes
        take any building index array: no map of 2 100 buildings is needed)"""
        rng = np.random.default_rng(21)
        n, npl, nb = 4097, 2100, 2100
        assert npl * (nb + 1) > 1 << 22
        plane, bidx = rng.integers(-1, npl + 2, n).astype(np.int32), rng.integers(-1, nb, n).astype(np.int32)
        v = ctx.plane_buildings(plane, bidx, npl, nb)
        _same_votes(v, bref.votes(plane, bidx, npl, nb))
        return v

    return out + [(f"assign_votes_{n}", assign_and_votes(n)) for n in (255, 257, 4097)] + [("votes_sorted_keys", votes_sorted_keys)]


@stage("roofs", order=("strip_129", "one_pixel_65"))
def _roofs():
    import test_gpu_roofs as R

    def one_pixel(n):
        xyz = np.tile(R.pts([(1, 1)]), (n, 1))
        xyz[:, 2] = 10 * np.arange(n) - 100
        return R.case(xyz, np.zeros((3, 3), np.int32), np.where(np.arange(n) % 3 == 2, 1, 2), 2, ground_th=-50.0)

    def strip(n):
        return R.case(R.pts([(0, 0), (n - 1, 0)]), np.zeros((1, n), np.int32), [5, 2], 5)

    cs = {f"one_pixel_{n}": one_pixel(n) for n in (1, 63, 65)}
    cs.update({f"strip_{n}": strip(n) for n in (9, 65, 129)})
    cs["no_planes"] = R.case(R.pts([(0, 0), (2, 1)]), np.array([[0, -1, 1], [0, 0, 1]], np.int32), [1, -1], 0)
    cs["no_building"] = R.case(R.pts([(0, 0), (1, 1)]), np.full((2, 3), -1, np.int32), [1, 1], 1)
    # planes above 2048 take the global-atomic path of both figure passes (test_more_planes_than_the_lds_tables, smaller)
    cs["more_planes_than_the_lds_tables"] = R._random_case(60, 60, 9000, 2300, 2300, block=6)
    assert (cs["more_planes_than_the_lds_tables"]["plane_idx"] > 2048).sum() > 50
    return [(k, lambda c, O, k=k: R.check(c, cs[k])) for k in cs]


@stage("plane_fit", order=("patches_4097", "sheet_65"))
def _fit():
    import test_gpu_plane_fit as F
    fc = F.fc

    def sheet(n):
        return lambda c, O: F.check(c, F.sheet(np.random.default_rng(n), n), np.ones(n, np.int32), 1)[0]

    def patches(n, m, kind, big_from=0):
        def f(ctx, O):
            rng = np.random.default_rng(n + m)
            xyz, plane = fc.patches(rng, n, m, spread=3000, big_from=big_from)
            xyz, plane = fc.layout(rng, xyz, plane, kind)
            got, want = F.check(ctx, xyz, plane, m)
            if m > fc.FIT_CAP:
                assert ("wave_global" if kind == "contiguous" else "lane_global") in fc.reach(dict(plane_idx=plane, n_planes=m), want)
            return got
        return f

    out = [(f"sheet_{n}", sheet(n)) for n in (1, 3, 63, 65)]
    out += [("patches_255", patches(255, 7, "random")), ("patches_257", patches(257, 7, "mixed")), ("patches_4097", patches(4097, 40, "mixed"))]
    # more planes than the LDS tables: whole waves of one label (wave_global) and every lane another plane (lane_global)
    out += [("wave_global", patches(9000, fc.FIT_CAP + 40, "contiguous", big_from=fc.FIT_CAP)),
            ("lane_global", patches(9000, fc.FIT_CAP + 40, "random", big_from=fc.FIT_CAP))]
    out.append(("no_planes", lambda c, O: F.check(c, F.sheet(np.random.default_rng(2), 10), np.zeros(10, np.int32), 0)[0]))
    return out


@stage("solids", order=("blob_65x64", "checkerboard"))
def _solids():
    import test_gpu_solids as S
    cs = dict(S.SHAPES)
    for w, h in ((1, 63), (63, 1), (65, 64), (31, 33), (257, 1)):
        cs[f"blob_{w}x{h}"] = S.cases.blob_case(w, h, seed=w * 1000 + h, size=7)
    flat = S.cases.blob_case(31, 17, seed=2)  # (no planes: everything is flat)
    cs["no_planes"] = S.cases.make(flat["bmap"], np.zeros((17, 31)), flat["n_buildings"], np.zeros((0, 3)), np.zeros((0, 3)), [], [], 10, 100,
                                   flat["flat"])
    out = [(k, lambda c, O, k=k: S.check(c, cs[k])) for k in cs]

    def with_bases(ctx, O):  # under bs_set_building_bases with one base for all: the scalar run at that base_z
        c = dict(cs["blob_65x64"], base_z=700)
        ctx.set_building_bases(np.full(c["n_buildings"], 700, np.int32))
        try:
            got = S.run(ctx, c)
        finally:
            ctx.set_building_bases(None)
        want = S.cases.run_ref(c)
        assert S.sr.same(got, want) is None, S.sr.same(got, want)
        return got

    return out + [("with_bases", with_bases)]


@stage("generalise", order=("strip_257", "island"))
def _generalise():
    import test_gpu_generalise as G
    names = ("one_pixel", "island", "two_small_facets", "strip_65", "strip_257", "strip_4097", "coplanar_merge_flat", "gable_is_a_ridge",
             "checkerboard_8")
    out = [(k, lambda c, O, k=k: G.check(c, G.SHAPES[k])) for k in names]
    empty = G.cases._shape(np.full((3, 4), -1), np.zeros((3, 4)), nb=0, min_pixels=3)
    return out + [("no_building", lambda c, O: G.check(c, empty))]


@stage("facets", order=("blob_65x33", "ring_with_hole"))
def _facets():
    import test_gpu_facets as F
    cs = {k: F.SHAPES[k] for k in ("one_pixel", "ring_with_hole", "serpentine", "gable", "plane_checkerboard")}
    for w, h in ((1, 33), (33, 1), (31, 33), (32, 33), (33, 15), (33, 16), (33, 17), (63, 33), (64, 33), (65, 33), (33, 257)):
        cs[f"blob_{w}x{h}"] = F.cases.blob_case(w, h, seed=w * 1000 + h, size=7)
    cs["no_building_pixel"] = F.cases.solid_fuzz_case(15)  # (the case of test_no_building_pixel)
    assert (cs["no_building_pixel"]["bmap"] < 0).all()
    return [(k, lambda c, O, k=k: F.check(c, cs[k])) for k in cs]


@stage("outlines", order=("serpentine", "two_holes"))
def _outlines():
    import test_gpu_outlines as L
    cs = {k: L.NAMED[k] for k in ("one_pixel", "two_holes", "serpentine", "strip_31", "strip_32", "full_image", "nothing")}
    for w, h in L.cases.LINE_SIZES:
        if max(w, h) >= 63:
            cs[f"line_{w}x{h}"] = L.cases.line_case(w, h)
    for w, h in ((31, 33), (33, 33)):
        cs[f"blob_{w}x{h}"] = L.cases.from_facet(L.fc.blob_case(w, h, seed=w * 1000 + h, size=7))
    return [(k, lambda c, O, k=k: L.check(c, cs[k], memo(("outlines", k), lambda: L.cases.run_ref(cs[k])))) for k in cs]


CHAIN = ("one_pixel", "nothing", "hole", "spiral", "noisy_diagonal", "line_1x63", "line_65x1", "random_8")


@stage("simplify", order=("spiral-25", "hole-0"))
def _simplify():
    import test_gpu_simplify as S

    def run(k, tol):
        return lambda c, O: S.check(c, S.NAMED[k], tol, memo(("simplify", k, tol), lambda: S.cases.run_ref(S.NAMED[k], tol)))

    return [(f"{k}-{tol[0]}", run(k, tol)) for k in CHAIN for tol in ((0, 1), (25, 4))]


def _uncross_check(ctx, c, tol, **kw):
    import test_gpu_uncross as U
    return U.check(ctx, c, tol, **kw)


@stage("clean", order=("spiral-25", "finger-1000000-cell1"))
def _clean():
    """uncross and the sweeps, the mode on and off"""
    import test_gpu_sweep as W
    import test_gpu_uncross as U
    out = [(f"{k}-{tol[0]}", lambda c, O, k=k, tol=tol: U.check(c, U.NAMED[k], tol)) for k in CHAIN for tol in ((0, 1), (25, 4))]
    for name, tol in (("random_20", (25, 4)), ("finger", (1000000, 1))):  # conflicting runs: one corner pair per cell, one cell
        for cl in (1, 30):
            out.append((f"{name}-{tol[0]}-cell{cl}", lambda c, O, name=name, tol=tol, cl=cl: U.check(c, U.NAMED[name], tol, cell_log2=cl,
                                                                                                    tops=(True,))))
    for name, tol in (("s_curve", (100, 1)), ("bay", (1000000, 1)), ("random_20", (25, 4))):
        for mode in (1, 2):
            out.append((f"sweep_{name}-{tol[0]}-mode{mode}", lambda c, O, name=name, tol=tol, mode=mode: W.check(c, name, tol, mode)))
    return out


@stage("triangles", order=("long_comb", "nested"))
def _triangles():
    import test_gpu_triangulate as T
    # (long_comb: the global workspace; sieve_24: the LDS workgroup)
    names = ("one_pixel", "nothing", "hole", "spiral", "nested", "sieve_24", "long_comb", "line_1x63", "line_65x1")
    return [(n, lambda c, O, n=n: T.check(c, n, T.RUNS[n][1][0], with_top=i % 2 == 0)) for i, n in enumerate(names)]


@stage("poly_solids", order=("sieve_24", "nested"))
def _poly():
    import test_gpu_polysolid as P
    names = ("one_pixel", "no_label_pixel", "hole", "nested", "wall_8", "sieve_24", "strip_1023", "strip_1025", "line_1x63")
    return [(n, lambda c, O, n=n: P.check(c, n, *P.variants(n)[0])) for n in names]


@stage("model_raster", order=("bay", "nested"))
def _model_raster():
    import test_gpu_modelraster as M
    names = ["one_pixel", "no_label_pixel", "bay", "staircase", "nested", "hole", "line_1x63", "line_65x1"]
    names += [f"strip_{n}" for n in M.cases.STRIPS if n < 2000]
    return [(n, lambda c, O, n=n: M.check(c, n, M.BY_NAME[n][1][-1 if n == "bay" else 0])) for n in names]


@stage("point_residuals", order=("fuzz_1", "nested"))
def _point_residuals():
    import test_gpu_pointresid as R
    names = ["bay", "staircase", "nested", R.NB_NAME, "fuzz_1", "pstrip_255", "pstrip_257"]
    return [(n, lambda c, O, n=n: R.check(c, n, R.BY_NAME[n][1][0])) for n in names]


@stage("terrain", order=("many", "min_ground"))
def _terrain():
    import test_gpu_terrain as T

    def run(n):
        def f(ctx, O):
            got, want = T.run(ctx, T.BY_NAME[n]), T.ref(n)[0]
            assert T.tref.same(got, want) is None, (n, T.tref.same(got, want))
            return got
        return f

    return [(n, run(n)) for n in ("none", "min_ground", "ranks_1_2", "two_close", "empty_ring", "early", "border", "many")]


@stage("ground", order=("odd", "tiny"))
def _ground():
    import test_gpu_ground as G

    def run(n):
        def f(ctx, O):
            got, want = G.run(ctx, G.BY_NAME[n]), G.ref(n)
            assert G.differs(got, want) is None, (n, G.differs(got, want))
            return got
        return f

    return [(n, run(n)) for n in ("tiny", "wide_window", "row", "column", "odd", "long_rows", "hole", "edge_equal", "sixteen")]


@stage("evidence", order=("tile_plus", "r1"))
def _evidence():
    import test_gpu_evidence as E

    def run(c, want):
        def f(ctx, O):
            got = E.run(ctx, c)  # (under the case's ground model: bs_set_ground_model, gm_dev)
            assert E.differs(got, want()) is None, (c["name"], E.differs(got, want()))
            return got
        return f

    out = [(n, run(E.BY_NAME[n], lambda n=n: E.ref(n))) for n in ("one_point", "no_planes", "all_below", "r0", "r1", "r15_narrow",
                                                                 "straddle_small", "share_boundary", "model")]
    # 31 / 32 / 33 wide for the 32 x 32 tiles of the window kernel
    return out + [(n, run(E.LARGE[n], lambda n=n: E.large_ref(n))) for n in ("tile_minus", "tile_exact", "tile_plus")]


@stage("sharded", order=("remap_rows_table", "remap_rows_search"))
def _sharded():
    """bs_segment_sharded with thread-ranks on bs_comm_local_create at world 2: every rank's context guarded (the run gets
    the first context from the test and makes the second the same way)"""
    import scenarios as S
    import test_gpu_sharded_scenarios as SS
    import thread_ranks as T

    def run(name):
        def f(ctx, O):
            sc = S.BY_NAME[name]
            assert sc.world == 2
            other = api.Context(0)
            try:
                other.selftest_scratch_guard(canary=True, poison=getattr(ctx, "_scratch_poison", None))
                with env(BS_COMM_LOCAL_TIMEOUT_S=str(T.COMM_TIMEOUT_S)):
                    comm = T.Comm(2)
                    try:
                        f_, parts, res = SS._run([ctx, other], comm, sc, O)
                    finally:
                        comm.close()
                SS._check(res, f_, sc, parts)
                clean(other)
            finally:
                other.close()
            return [(lab, {k: v for k, v in info.items() if not k.startswith("ms_")}, pls) for lab, info, pls in res]
        return f

    def remap_rows(n_rows):  # (bs_remap_rows_dev: the binary search, and from 2^22 entries on the look-up table, sh[24])
        return lambda ctx, O: _remap_rows(ctx, n_rows)

    return [(n, run(n)) for n in ("boxes3_contiguous_w2", "boxes3_k15_w2", "disc_lattice_retry4_w2")] + \
           [("remap_rows_search", remap_rows(4097)), ("remap_rows_table", remap_rows((1 << 22) // 16))]


def _remap_rows(ctx, n_rows):
    import torch
    rng = np.random.default_rng(5)
    sg = np.sort(rng.choice(100_000, 5_000, replace=False)).astype(np.int32)
    rows = sg[rng.integers(0, len(sg), (n_rows, 16))]
    d_sg, d_rows = torch.from_numpy(sg).cuda(), torch.from_numpy(rows).cuda()
    d_out = torch.empty_like(d_rows)
    torch.cuda.synchronize()
    assert ctx.remap_rows_dev(d_rows.data_ptr(), len(rows), 16, d_sg.data_ptr(), len(sg), d_out.data_ptr()) == 0
    got = d_out.cpu().numpy()
    assert np.array_equal(sg[got], rows)
    return got


def _cases(name):
    return memo(("cases", name), STAGES[name])


def _run_all(name, ctx, oracle):
    """every case of the stage on ONE context, in the listed order: later cases meet the buffers of the earlier ones"""
    return [(cid, run(ctx, oracle)) for cid, run in _cases(name)]


def _run_each_fresh(name, oracle, poison):
    """every case of the stage on a context of its own.  A buffer made for a larger case reports that case's request, so a
    smaller case after it would take the early return of reserve: its overrun would land inside the larger request and
    nothing would be poisoned again.  On its own context every case meets guards behind exactly its own requests."""
    out = []
    for cid, run in _cases(name):
        with guarded(poison) as ctx:
            out.append((cid, run(ctx, oracle)))
            assert ctx.selftest_scratch_check()["n_guarded"] > 0, cid
    return out


# ---- a. the check itself ----------------------------------------------------------------------------------------------
def _poke(address, offset, value=0x11):
    from ctypes import c_void_p
    hip = _hip()
    assert hip.hipMemset(c_void_p(address + offset), value, 1) == 0 and hip.hipDeviceSynchronize() == 0


def _hip():
    """the HIP runtime the product library is linked against, through the library's own handle (dlsym on a handle also
    searches its dependencies): the very instance the contexts allocate with"""
    import ctypes
    h = _lib.load()
    h.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    h.hipMemset.restype = ctypes.c_int
    h.hipDeviceSynchronize.restype = ctypes.c_int
    return h


def test_the_check_names_the_buffer_and_the_damaged_bytes(oracle):
    """one byte written at the first and at the last guard byte of one buffer is reported with that buffer's name and
    offsets; the last requested byte is not; all three writes lie inside the allocation"""
    _torch_first()
    with api.Context(0) as ctx:
        ctx.selftest_scratch_guard(canary=True)
        ctx.knn_normals(synth.uniform(257, seed=1), api.default_params(k=15))
        rep = ctx.selftest_scratch_check()
        slots = ctx.selftest_scratch_list()
        assert rep["n_damaged"] == 0 and rep["n_guarded"] == len(slots) > 5 and rep["bytes_requested"] > 257 * 15 * 4
        for s in slots:
            assert s["guard"] == max(4096, s["requested"] // 8 + 256) and s["requested"] > 0 and s["address"] != 0
        s = next(s for s in slots if s["name"] == "spts")
        assert not s["host"]
        _poke(s["address"], s["requested"] - 1)  # the last byte of the request
        assert ctx.selftest_scratch_check()["n_damaged"] == 0
        _poke(s["address"], s["requested"])      # the first guard byte
        rep = ctx.selftest_scratch_check()
        assert rep["n_damaged"] == 1 and len(rep["damaged"]) == 1
        d = rep["damaged"][0]
        assert (d["name"], d["requested"], d["first_bad"], d["last_bad"]) == ("spts", s["requested"], 0, 0), describe(rep)
        _poke(s["address"], s["requested"], _lib_canary())  # (mended)
        assert ctx.selftest_scratch_check()["n_damaged"] == 0
        _poke(s["address"], s["requested"] + s["guard"] - 1)  # the last guard byte
        d = ctx.selftest_scratch_check()["damaged"][0]
        assert (d["name"], d["first_bad"], d["last_bad"]) == ("spts", s["guard"] - 1, s["guard"] - 1)
        other = next(t for t in slots if t["name"] == "table")
        _poke(other["address"], other["requested"] + 7)
        rep = ctx.selftest_scratch_check()
        assert rep["n_damaged"] == 2 and [d["name"] for d in rep["damaged"]] == ["table", "spts"]  # (the order of bs_ctx)
        assert "table: requested" in describe(rep) and "+7 .. +7" in describe(rep)


def _lib_canary():
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "bs_common.h")).read()
    assert "SCRATCH_CANARY = 0xC5" in src
    return 0xC5


def test_the_guard_is_refused_once_the_context_has_allocated_and_leaves_other_contexts_alone():
    _torch_first()
    xyz, p = synth.uniform(300, seed=2), api.default_params(k=15)
    with api.Context(0) as g, api.Context(0) as plain:
        g.selftest_scratch_guard(canary=True, poison=POISON[0])
        g.knn_normals(xyz, p)
        plain.knn_normals(xyz, p)
        with pytest.raises(api.BsError) as e:
            g.selftest_scratch_guard(canary=True)
        assert e.value.status == -1 and "already allocated" in str(e.value)
        with pytest.raises(api.BsError) as e:
            plain.selftest_scratch_guard(canary=True)
        assert e.value.status == -1
        # the unguarded context beside it allocates as always: nothing of it is listed or counted
        assert plain.selftest_scratch_list() == [] and plain.selftest_scratch_check()["n_guarded"] == 0
        assert len(g.selftest_scratch_list()) > 5
    with api.Context(0) as c:
        for bad in (dict(flags=4, poison=0), dict(flags=1, poison=256), dict(flags=1, poison=-1)):
            assert c._L.bs_selftest_scratch_guard(c._h, bad["flags"], bad["poison"]) == -1
        assert c._L.bs_selftest_scratch_check(c._h, None) == -1


def test_a_kept_buffer_is_not_poisoned_again():
    """a request up to the size a buffer was made for keeps the buffer and its contents (the early return of reserve): the
    bases set before a larger and a smaller call survive, and a fresh allocation reports its request, not more"""
    _torch_first()
    with guarded(POISON[1]) as ctx:
        base = np.arange(100, dtype=np.int32) * 3
        ctx.set_building_bases(base)
        a = {s["name"]: s for s in ctx.selftest_scratch_list()}
        assert a["bases_dev"]["requested"] == 400
        ctx.set_building_bases(base[:10])
        b = {s["name"]: s for s in ctx.selftest_scratch_list()}
        assert b["bases_dev"]["address"] == a["bases_dev"]["address"] and b["bases_dev"]["requested"] == 400
        assert np.array_equal(ctx.building_bases(), base[:10])
        ctx.set_building_bases(np.arange(101, dtype=np.int32))
        assert {s["name"]: s for s in ctx.selftest_scratch_list()}["bases_dev"]["requested"] == 404


# ---- b. canary, d. poison ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(STAGES))
def test_canary(oracle, name):
    """canary only, a fresh context per case"""
    _run_each_fresh(name, oracle, None)


@pytest.mark.parametrize("name", list(STAGES))
def test_poison(oracle, name):
    """POISON[0] on a fresh context per case; POISON[1] on one context for the whole stage, where the cases also meet
    what the cases before them left; byte-identical results"""
    runs = [_run_each_fresh(name, oracle, POISON[0])]
    with guarded(POISON[1]) as ctx:
        runs.append(_run_all(name, ctx, oracle))
    for (cid, a), (_, b) in zip(*runs):
        assert first_difference(a, b) is None, f"{name} / {cid}: {first_difference(a, b)} depends on what the scratch held"


# ---- e. order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ORDER))
def test_order(oracle, name):
    """A, B, A and B, A, B on one poisoned context each: equal to the references every time (the runs assert it), equal
    to each other, and no guard damaged"""
    by_id = dict(_cases(name))
    a, b = (by_id[k] for k in ORDER[name])
    seen = {0: [], 1: []}
    for poison, seq in ((POISON[0], (0, 1, 0)), (POISON[1], (1, 0, 1))):
        with guarded(poison) as ctx:
            for i in seq:
                seen[i].append((a, b)[i](ctx, oracle))
    for i, runs in seen.items():
        for r in runs[1:]:
            assert first_difference(runs[0], r) is None, f"{name} / {ORDER[name][i]}: {first_difference(runs[0], r)} depends on the call before"


# ---- c. capacity limits -----------------------------------------------------------------------------------------------
# one cloud per engine and limit: the smallest input of tests/test_gpu_grow_limits.py that makes the counter positive there
LIMITS = [
    ("v2", "fuzz_7_106", dict(max_waves=7), "rounds_capped"), ("v1", "fuzz_7_106", dict(max_waves=7), "rounds_capped"),
    ("k32", "boxes_k32", dict(max_waves=7), "rounds_capped"),
    ("v2", "facade400_k16", dict(pool_cap=898984), "attempts_nomem"), ("v1", "facade400_k16", dict(pool_cap=898984), "attempts_nomem"),
    ("k32", "boxes_k32", dict(pool_cap=169705), "attempts_nomem"),
    ("v2", "fuzz_7_106", dict(max_pending=1), "dropped_pend_count"), ("v1", "fuzz_7_106", dict(max_pending=1), "dropped_pend_count"),
    ("k32", "fuzz_2718_16", dict(max_pending=1), "dropped_pend_count"),
    ("v2", "fuzz_7_106", dict(pstore_cap=3000), "dropped_pend_store"), ("v1", "fuzz_7_106", dict(pstore_cap=3000), "dropped_pend_store"),
    ("k32", "fuzz_2718_16", dict(pstore_cap=3000), "dropped_pend_store"),
]


@pytest.mark.parametrize("engine,name,lim,counter", LIMITS, ids=[f"{e}-{n}-{next(iter(l))}" for e, n, l, _ in LIMITS])
def test_limits(oracle, engine, name, lim, counter):
    """canary alone, then canary + both poisons: the grow equals the oracle (asserted by _grow), the counter is positive,
    no guard is damaged"""
    import test_gpu_grow_limits as GL
    with env(**({"BS_GROW_V2": "0"} if engine == "v1" else {})):
        for poison in (None,) + POISON:
            with guarded(poison) as ctx:
                gc = GL._grow(ctx, oracle, name, lim, f"guard[{engine}]", unhooked_after=False)
                assert gc[counter] > 0, gc


# ---- f. coverage ------------------------------------------------------------------------------------------------------
# slots of a group that no case of this module allocates, each with the path that would need it ("Guarded
# scratch"): only paths that need more than test size or more than one GPU may stand here
UNREACHED = {}


def _groups():
    import ctypes as C
    import re
    src = open(os.path.join(os.path.dirname(api.__file__), "csrc", "bs_capi.hip")).read()
    table = src[src.index("void scratch_members("):src.index("#undef BS_ONE")]
    groups = [g for g in re.findall(r"BS_(?:ONE|ARR)\((\w+)\)", table) if g != "m"] + ["rg_hout"]
    n = C.c_int64(0)
    assert _lib.load().bs_selftest_scratch_list(None, None, 0, C.byref(n)) == 0
    return sorted(set(groups)), n.value


def test_every_member_group_was_allocated_under_guard():
    """runs last in the module: every array and every single buffer of bs_ctx was allocated under guard, and checked
    clean, by some test above; the slots of a group that nothing reached are printed"""
    groups, n_members = _groups()
    assert len(groups) > 60 and n_members > 400
    if not _ALLOCATED:
        pytest.fail("no test of this module ran before the coverage assertion")
    from test_scratch_table_cpu import _declared_buffers
    sizes = dict(_declared_buffers())
    assert sorted(sizes) == groups and sum(sizes.values()) == n_members
    missing = [g for g in groups if g not in _ALLOCATED]
    unreached = {f"{g}[{i}]" for g in groups if sizes[g] > 1 for i in range(sizes[g]) if i not in _ALLOCATED.get(g, ())}
    print("slots no case of this module allocates:", sorted(unreached))
    assert not missing, f"bs_ctx members never allocated under guard: {missing}"
    assert unreached == set(UNREACHED), (sorted(unreached - set(UNREACHED)), sorted(set(UNREACHED) - unreached))
