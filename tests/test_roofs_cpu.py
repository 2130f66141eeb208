"""Roofs (include/bs_api.h, "roofs") without a GPU: the C-ABI surface, the two host-only calls (bs_roof_homes,
bs_roofs_write_obj) against their restatement, the numpy restatement tests/roof_ref against a pure-Python brute force,
the gabled scene through the CPU oracle's labels, and the coverage of the fuzz cases the device suite runs."""
import ctypes as C
import importlib.util
import os
import sys
from collections import Counter, deque
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
sys.path.insert(0, os.path.join(HERE, "building_ref"))
sys.path.insert(0, os.path.join(HERE, "roof_ref"))
import building_ref as bref  # noqa: E402
import fuzz_cases as fz  # noqa: E402
import ref  # noqa: E402
import roof_ref as rr  # noqa: E402

from buildingsegment_amd import api  # noqa: E402


def load_roof_scenes():
    """tests/roof_ref/scenes.py under a name of its own (tests/building_ref has a scenes.py too)"""
    if "roof_scenes" not in sys.modules:
        spec = importlib.util.spec_from_file_location("roof_scenes", os.path.join(HERE, "roof_ref", "scenes.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["roof_scenes"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["roof_scenes"]


NEW = ["bs_roof_homes", "bs_roofs_dev", "bs_roofs", "bs_roofs_free", "bs_roofs_write_obj"]


def test_new_symbols_are_declared_loaded_and_exported():
    from buildingsegment_amd import _lib, build
    import test_abi
    build.build()
    L = _lib.load()
    declared = test_abi._declared()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.bs_api_version() == 5
    st = _lib.Roofs()
    L.bs_roofs_free(C.byref(st))  # a zeroed struct is accepted
    assert st.n_planes == 0 and not st.pixels
    for name in ("roof_homes", "write_roofs_obj", "Roofs"):
        assert hasattr(api, name), name
    for name in ("roofs", "roofs_dev", "roof_model"):
        assert hasattr(api.Context, name), name


def test_roof_homes_match_the_restatement():
    nan = float("nan")
    normal = np.array([[0, 0, 1.0], [0, 0, 0.5], [0, 0, np.nextafter(0.5, 0)], [0.6, 0, 0.8], [0, 0, nan], [nan, 0, 0.9],
                       [0, 0, 1.0], [0, 0, 1.0], [0, 0, 1.0], [0, 0, -1.0], [0, 0, 1.0]])
    pb = np.array([3, 0, 0, 7, 1, 2, -1, 4, 4, 5, 6], np.int32)
    vin = np.array([10, 6, 6, 1, 9, 9, 0, 5, 5, 8, 0], np.int64)
    tot = np.array([11, 11, 11, 1, 9, 9, 4, 10, 9, 8, 0], np.int64)
    want = [3, 0, -1, 7, -1, 2, -1, -1, 4, -1, -1]  # [7]: the exact half; [10]: no point at all
    got = api.roof_homes(normal, pb, vin, tot)
    assert got.dtype == np.int32 and got.tolist() == want == rr.homes(normal, pb, vin, tot).tolist()
    assert api.roof_homes(normal, pb, vin, tot, min_normal_z=0.9).tolist() == rr.homes(normal, pb, vin, tot, 0.9).tolist()
    assert api.roof_homes(normal, pb, vin, tot, min_normal_z=-2.0).tolist() == [3, 0, 0, 7, -1, 2, -1, -1, 4, 5, -1]
    rng = np.random.default_rng(5)
    for _ in range(20):
        n = int(rng.integers(0, 40))
        nrm = rng.normal(size=(n, 3))
        nrm[rng.random(n) < 0.2, 2] = nan
        pb = rng.integers(-1, 5, n).astype(np.int32)
        tot = rng.integers(0, 20, n)
        vin = np.minimum(rng.integers(0, 20, n), tot)
        vin[rng.random(n) < 0.3] = 0
        assert api.roof_homes(nrm, pb, vin, tot).tolist() == rr.homes(nrm, pb, vin, tot).tolist()
    assert api.roof_homes(np.zeros((0, 3)), [], [], []).shape == (0,)
    with pytest.raises(ValueError):
        api.roof_homes(np.zeros((2, 3)), [0], [1, 1], [1, 1])


# ---- the OBJ writer ------------------------------------------------------------------------------------------------
# Two buildings adjacent in the map (columns 0-3 and 4-7), runs that end at the image edge, a gap, every kind of plane.
OBJ_MAP = np.array([[0, 0, 0, 0, 1, 1, 1, 1],
                    [0, 0, 0, 0, 1, 1, 1, 1],
                    [-1, 0, 0, -1, 1, 1, -1, 1],
                    [2, 2, 2, 2, 2, 2, 2, 2]], np.int32)
OBJ_ROOF = np.array([[1, 1, 2, 2, 2, 2, 3, 3],     # plane 2 runs across the border of the buildings: two runs
                     [1, 1, 1, 0, 4, 4, 4, 4],     # an unroofed pixel; a run to the right edge
                     [-1, 5, 5, -1, 6, 6, -1, 6],
                     [7, 7, 7, 7, 7, 7, 7, 7]], np.int32)  # one run over the whole row
OBJ_NORMAL = np.array([[0, 0, 1.0],          # 1 flat: H == cz
                       [0.6, 0, 0.8],        # 2 sloped, inside its clamps
                       [0.9, 0.3, 0.1],      # 3 steep: clamps at both ends
                       [0.5, 0.5, 0.0],      # 4 nz == 0: +-inf or NaN, clamped
                       [0.1, np.nan, 0.9],   # 5 NaN: z_min
                       [0.2, -0.1, -0.7],    # 6 nz < 0 is not an error
                       [-0.3, 0.2, 0.9]])    # 7
OBJ_CENTER = np.array([[50, 50, 3333], [300, 20, 4000], [650, 50, 5000], [600, 150, 2000], [150, 250, 2500],
                       [500, 250, 2600], [400, 350, -700]], np.int32)
OBJ_ZMIN = np.array([3000, 3000, 4990, 1900, 2400, 2590, -800], np.int32)
OBJ_ZMAX = np.array([3500, 5000, 5010, 2100, 2600, 2610, -600], np.int32)
OBJ_PIXELS = np.array([5, 4, 2, 4, 2, 3, 8], np.int64)


def _obj_roofs(n=7):
    z = np.zeros
    return api.Roofs(n, 8, 4, 0, 0, 0, 0, OBJ_PIXELS[:n].copy(), z(n, np.int64), z((n, 4), np.int32), z(n, np.int64),
                     OBJ_ZMIN[:n].copy(), OBJ_ZMAX[:n].copy(), z(n, np.int64), normal=OBJ_NORMAL[:n], center=OBJ_CENTER[:n])


@pytest.mark.parametrize("origin", [None, (0, 0, 0), (431200, 5620000, 87000), (-4321, -99, -20)],
                         ids=["null", "zero", "positive", "negative"])
@pytest.mark.parametrize("bin_", [1, 37, 100])
def test_write_obj_bytes_equal_the_restatement(tmp_path, origin, bin_):
    api.write_roofs_obj(_obj_roofs(), OBJ_MAP, tmp_path / "r.obj", origin=origin, roof=OBJ_ROOF, bin=bin_)
    got = (tmp_path / "r.obj").read_bytes()
    want = rr.obj_text(OBJ_ROOF, OBJ_MAP, OBJ_PIXELS, OBJ_ZMIN, OBJ_ZMAX, OBJ_NORMAL, OBJ_CENTER, bin_, origin)
    assert got == want
    runs = rr.runs_of(OBJ_ROOF, OBJ_MAP)
    assert len(runs) == 10 and (0, 2, 3, 2) in runs and (0, 4, 5, 2) in runs and (1, 4, 7, 4) in runs and (3, 0, 7, 7) in runs
    assert got.startswith(b"# roof runs: 10 over 7 planes\n") and got.endswith(b"f 37 38 39 40\n")
    assert got.count(b"\nv ") == 40 and got.count(b"\nf ") == 10
    if bin_ == 100:  # the kinds of plane the case is there for, on the restatement's own heights
        o = np.zeros(3, np.int64) if origin is None else np.asarray(origin, np.int64)
        v = np.array([ln.split()[1:] for ln in got.decode().splitlines() if ln.startswith("v ")], np.int64) - o
        by_run = v.reshape(10, 4, 3)
        k = {r: i for i, r in enumerate(runs)}
        assert (by_run[k[(0, 0, 1, 1)], :, 2] == 3333).all()  # flat: cz
        steep = by_run[k[(0, 6, 7, 3)], :, 2]
        assert steep.min() == 4990 and steep.max() == 5010  # both clamps
        assert set(by_run[k[(1, 4, 7, 4)], :, 2]) <= {1900, 2100}  # nz == 0
        assert (by_run[k[(2, 1, 2, 5)], :, 2] == 2400).all()  # NaN: z_min
        assert (by_run[k[(0, 4, 5, 2)], 1, :2] == [600, 0]).all() and (by_run[k[(1, 4, 7, 4)], 2, :2] == [800, 200]).all()


def test_write_obj_edges_and_errors(tmp_path):
    r = _obj_roofs()
    api.write_roofs_obj(r, np.full((4, 8), -1, np.int32), tmp_path / "none.obj", roof=np.full((4, 8), -1, np.int32))
    assert (tmp_path / "none.obj").read_bytes() == b"# roof runs: 0 over 7 planes\n"
    empty = api.Roofs(0, 8, 4, 0, 0, 0, 0, *(np.zeros(0, np.int64),) * 2, np.zeros((0, 4), np.int32), np.zeros(0, np.int64),
                      np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), normal=np.zeros((0, 3)),
                      center=np.zeros((0, 3), np.int32))
    api.write_roofs_obj(empty, OBJ_MAP, tmp_path / "e.obj", roof=np.where(OBJ_MAP < 0, -1, 0).astype(np.int32))
    assert (tmp_path / "e.obj").read_bytes() == b"# roof runs: 0 over 0 planes\n"
    with pytest.raises(api.BsError) as e:  # a roof value above n_planes
        api.write_roofs_obj(_obj_roofs(6), OBJ_MAP, tmp_path / "x.obj", roof=OBJ_ROOF)
    assert e.value.status == -1
    with pytest.raises(api.BsError):
        api.write_roofs_obj(r, OBJ_MAP, tmp_path / "x.obj", roof=OBJ_ROOF, bin=0)
    with pytest.raises(api.BsError):
        api.write_roofs_obj(r, OBJ_MAP, tmp_path / "no_such_dir" / "x.obj", roof=OBJ_ROOF)
    with pytest.raises(ValueError):
        api.write_roofs_obj(r, OBJ_MAP[:2], tmp_path / "x.obj", roof=OBJ_ROOF)


# ---- the restatement against a brute force -------------------------------------------------------------------------
def _brute(xyz, bmap, plane, n_planes, home, bin_, th, min_votes):
    """per-pixel dicts for the vote, a breadth-first search by rounds for the fill, loops for the figures"""
    h, w = bmap.shape
    counts = {}
    counting = []
    for i, (x, y, z) in enumerate(xyz.tolist()):
        p = int(plane[i])
        px, py = x // bin_, y // bin_
        ok = (not z < th) and 1 <= p <= n_planes and bmap[py, px] >= 0 and home[p - 1] == bmap[py, px]
        counting.append(ok)
        if ok:
            counts.setdefault((py, px), {}).setdefault(p, 0)
            counts[(py, px)][p] += 1
    roof = [[-1 if bmap[y, x] < 0 else 0 for x in range(w)] for y in range(h)]
    support = [[0] * w for _ in range(h)]
    for (y, x), d in counts.items():
        best = max(d.values())
        if best >= min_votes:
            roof[y][x] = min(p for p, c in d.items() if c == best)
            support[y][x] = best
    frontier = deque((y, x) for y in range(h) for x in range(w) if roof[y][x] > 0)
    rounds = 0
    while frontier:
        reached = {}
        for y, x in frontier:
            for ny, nx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                if 0 <= ny < h and 0 <= nx < w and roof[ny][nx] == 0 and bmap[ny, nx] == bmap[y, x]:
                    reached[(ny, nx)] = min(reached.get((ny, nx), 1 << 40), roof[y][x])
        for (y, x), p in reached.items():
            roof[y][x] = p
        rounds += bool(reached)
        frontier = deque(reached)
    fig = {p: dict(n=0, zmin=rr.I32_MAX, zmax=rr.I32_MIN, zsum=0, pix=0, seed=0, box=[rr.I32_MAX, rr.I32_MAX, rr.I32_MIN, rr.I32_MIN])
           for p in range(1, n_planes + 1)}
    for i, (x, y, z) in enumerate(xyz.tolist()):
        p = int(plane[i])
        if counting[i] and roof[y // bin_][x // bin_] == p:
            f = fig[p]
            f["n"], f["zsum"], f["zmin"], f["zmax"] = f["n"] + 1, f["zsum"] + z, min(f["zmin"], z), max(f["zmax"], z)
    for y in range(h):
        for x in range(w):
            if roof[y][x] > 0:
                f = fig[roof[y][x]]
                f["pix"] += 1
                f["seed"] += support[y][x] > 0
                b = f["box"]
                f["box"] = [min(b[0], x), min(b[1], y), max(b[2], x), max(b[3], y)]
    return np.array(roof, np.int32).reshape(h, w), np.array(support, np.int32).reshape(h, w), rounds, fig


def test_restatement_against_a_brute_force_on_random_images():
    rng = np.random.default_rng(77)
    seen_rounds = Counter()
    for case in range(50):
        h, w = (int(rng.integers(1, 13)) for _ in range(2))
        nb = int(rng.integers(1, 4))
        bmap = rng.integers(-1, nb, (h, w)).astype(np.int32)
        if case % 3 == 0:
            bmap[:] = np.where(rng.random((h, w)) < 0.15, -1, 0)  # one building: longer fills
        n_planes = int(rng.integers(0, 6))
        bin_ = int(rng.choice([1, 3, 10]))
        n = int(rng.integers(1, 40 if case % 2 else 400))
        xyz = np.stack([rng.integers(0, w * bin_, n), rng.integers(0, h * bin_, n), rng.integers(-5, 30, n)], 1).astype(np.int32)
        plane = rng.integers(-1, n_planes + 2, n).astype(np.int32)
        home = rng.integers(-1, nb, n_planes).astype(np.int32)
        th, mv = float(rng.choice([0.0, 10.0, 10.5])), int(rng.choice([1, 2, 3]))
        nrm, ctr = rng.normal(size=(n_planes, 3)), rng.integers(0, 50, (n_planes, 3)).astype(np.int32)
        r = rr.roofs(xyz, bmap, plane, n_planes, home, nrm, ctr, bin_, th, mv)
        roof, support, rounds, fig = _brute(xyz, bmap, plane, n_planes, home, bin_, th, mv)
        assert np.array_equal(r.roof, roof) and np.array_equal(r.support, support) and r.fill_rounds == rounds, case
        for p in range(1, n_planes + 1):
            f = fig[p]
            assert (r.n_support[p - 1], r.z_min[p - 1], r.z_max[p - 1], r.z_sum[p - 1], r.pixels[p - 1], r.seed_pixels[p - 1]) == \
                (f["n"], f["zmin"], f["zmax"], f["zsum"], f["pix"], f["seed"]), (case, p)
            assert r.bbox[p - 1].tolist() == f["box"], (case, p)
        assert r.seeded_pixels == (support > 0).sum() and r.unroofed_pixels == (roof == 0).sum()
        assert r.filled_pixels == (roof > 0).sum() - r.seeded_pixels
        for y, x in zip(*np.nonzero(roof > 0)):  # the height, with Python's own floats
            p = roof[y, x] - 1
            X, Y = float(x * bin_ + bin_ // 2), float(y * bin_ + bin_ // 2)
            t = float(nrm[p, 0]) * (X - float(ctr[p, 0])) + float(nrm[p, 1]) * (Y - float(ctr[p, 1]))
            z = float(ctr[p, 2]) - t / float(nrm[p, 2])
            if not z >= r.z_min[p]:
                z = float(r.z_min[p])
            if z > r.z_max[p]:
                z = float(r.z_max[p])
            assert r.height[y, x] == int(z), (case, y, x)
        assert (r.height[roof <= 0] == rr.I32_MIN).all()
        seen_rounds[rounds] += 1
    assert max(seen_rounds) >= 4 and seen_rounds[0] > 0


def test_fill_is_synchronous_not_an_in_place_sweep():
    bmap = np.zeros((1, 9), np.int32)
    seed = np.array([[5, 0, 0, 0, 0, 0, 0, 0, 2]], np.int32)
    roof, rounds = rr.fill(seed, bmap)
    assert roof.tolist() == [[5, 5, 5, 5, 2, 2, 2, 2, 2]] and rounds == 4  # (a raster sweep would give 5 5 5 5 5 5 5 5 2)


# ---- the gabled scene through the CPU oracle's labels --------------------------------------------------------------
@pytest.fixture(scope="module")
def gabled(oracle):
    sc = load_roof_scenes()
    xyz = sc.gabled()
    neigh, normals = oracle.knn_normals(xyz, k=15)
    plane_idx, pl = oracle.region_grow(xyz, normals, neigh)
    img, th = oracle.grid_picture(xyz)
    _, mask = ref.footprints(img)
    b = bref.building_map(mask)
    a = bref.assign(xyz, b.map, b.n_buildings, 100, th)
    n_planes = len(pl["id"])
    pb, vin, tot, _ = bref.votes(plane_idx, a.building_idx, n_planes, b.n_buildings)
    home = rr.homes(pl["normal"], pb, vin, tot)
    r = rr.roofs(xyz, b.map, plane_idx, n_planes, home, pl["normal"], pl["center"], 100, th, 1)
    return SimpleNamespace(sc=sc, xyz=xyz, plane_idx=plane_idx, planes=pl, n_planes=n_planes, b=b, home=home, r=r, th=th)


def check_gabled_facts(sc, bmap, n_buildings, home, normal, center, plane_idx, n_planes, r):
    """what the scene is there for (shared with the device's end-to-end test)"""
    assert n_buildings == 3
    row, cols = sc.gable_pixels()
    gable = int(bmap[row, cols[0]])
    assert gable >= 0 and (bmap[row, cols] == gable).all()
    halves = [p for p in range(n_planes) if abs(normal[p, 0]) > 0.2 and normal[p, 2] > 0.8]
    assert len(halves) == 2 and normal[halves[0], 0] * normal[halves[1], 0] < 0  # the two slopes face each other
    assert [int(home[p]) for p in halves] == [gable, gable]
    for p in range(n_planes):  # no ground plane and no wall plane has a home
        if center[p, 2] < 1000 or normal[p, 2] < 0.5:
            assert home[p] == -1, p
    assert sorted(home[home >= 0].tolist()) == sorted([0, 1, 2, gable])
    assert (plane_idx == n_planes + 1).any()  # orphans of a plane that never committed: ignored
    assert r.unroofed_pixels == 0 and (r.roof[bmap >= 0] > 0).all() and (r.roof[bmap < 0] == -1).all()
    assert r.filled_pixels > 0 and 1 <= r.fill_rounds <= 6
    for p in range(n_planes):
        if home[p] >= 0:  # a roof plane lies in its own building only
            assert (bmap[r.roof == p + 1] == home[p]).all()
        else:
            assert r.pixels[p] == 0
    hgt = r.height[row, cols]
    top = int(np.argmax(hgt))
    assert abs(int(hgt[top]) - sc.RIDGE) <= 100 and abs(int(hgt[0]) - sc.EAVES) <= 100 and abs(int(hgt[-1]) - sc.EAVES) <= 100
    assert (np.diff(hgt[:top + 1]) >= 0).all() and (np.diff(hgt[top:]) <= 0).all()  # up to the ridge, then down
    assert set(r.roof[row, cols].tolist()) == {halves[0] + 1, halves[1] + 1}


def test_gabled_scene_through_the_oracle_labels(gabled):
    g = gabled
    assert g.n_planes == 6
    check_gabled_facts(g.sc, g.b.map, g.b.n_buildings, g.home, g.planes["normal"], g.planes["center"], g.plane_idx,
                       g.n_planes, g.r)


def test_gabled_scene_obj_text(gabled):
    g = gabled
    txt = rr.obj_text(g.r.roof, g.b.map, g.r.pixels, g.r.z_min, g.r.z_max, g.planes["normal"], g.planes["center"], 100,
                      (1000, 2000, 50)).decode().splitlines()
    runs = rr.runs_of(g.r.roof, g.b.map)
    assert txt[0] == f"# roof runs: {len(runs)} over 4 planes" and len(txt) == 1 + 5 * len(runs)
    z = np.array([ln.split()[3] for ln in txt[1:1 + 4 * len(runs)]], np.int64) - 50
    assert z.min() >= g.sc.EAVES - 100 and z.max() <= g.sc.RIDGE + 100


# ---- the fuzz cases of the device suite reach every regime ---------------------------------------------------------
def test_fuzz_cases_reach_every_regime():
    seen, none = Counter(), 0
    for seed in range(fz.N_CASES):
        c = fz.fuzz_case(seed)
        h, w = c["bmap"].shape
        assert h <= 150 and w <= 150 and len(c["xyz"]) <= 30000
        g = fz.regimes(c, fz.run_ref(c))
        seen.update(g)
        none += not g
    for k in fz.ALL_REGIMES:
        assert seen[k] >= 3, (k, seen[k])
    assert none >= 1
    assert fz.N_CASES == 40
