"""The terrain stage without a GPU (include/bs_api.h, "terrain"): the numpy restatement of the device layout against the
brute force of the definition, every image and figure with ==; what every case is there for; the errors of the definition;
and the names in the header and the loader."""
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_terrain_dev", "bs_terrain", "bs_terrain_free", "bs_set_building_bases", "bs_get_building_bases"]


def load_terrain_cases():
    if "terrain_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("terrain_cases", os.path.join(HERE, "terrain_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["terrain_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["terrain_cases"]


cases = load_terrain_cases()
tref, brute = cases.tref, cases.brute
BY_NAME = cases.BY_NAME
_REF, _BIG = {}, []


def ref(name):
    """(the restatement's result, its trace), computed once and never changed"""
    if name not in _REF:
        trace = {}
        _REF[name] = (tref.terrain(*cases.args(BY_NAME[name]), trace=trace), trace)
    return _REF[name]


def big():
    """(the case of about 600 000 points, the restatement's result, its trace), computed once"""
    if not _BIG:
        c, trace = cases.big(), {}
        _BIG.extend([c, tref.terrain(*cases.args(c), trace=trace), trace])
    return _BIG


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert re.search(r"^struct bs_terrain \{", txt, flags=re.M)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("terrain", "terrain_dev", "set_building_bases", "building_bases"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "Terrain") and "base" in api.Solids.__dataclass_fields__
    assert L.bs_api_version() == 5
    for macro, mine, refs in (("MAX_RING", _lib.TERRAIN_MAX_RING, tref.MAX_RING), ("FIG_CAP", _lib.TERRAIN_FIG_CAP, tref.FIG_CAP),
                              ("GRID", _lib.TERRAIN_GRID, tref.GRID)):
        v, = re.findall(r"^#define BS_TERRAIN_%s (\d+)" % macro, txt, flags=re.M)
        assert int(v) == mine == refs, macro
    # the struct of the loader follows the header field for field
    body = re.search(r"^struct bs_terrain \{(.*?)^\};", txt, flags=re.M | re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.Terrain._fields_]
    # and the dataclass carries every field of the references
    assert set(tref.DEVICE_FIELDS) <= set(api.Terrain.__dataclass_fields__)


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_references_agree(name):
    """the restatement of the layout equals the brute force of the definition in every image and figure, and what the
    header promises holds"""
    a = ref(name)[0]
    b = brute.terrain(*cases.args(BY_NAME[name]))
    assert brute.same(a, b) is None, brute.same(a, b)
    ok = a.status == 0
    assert (a.ground_min[ok] <= a.ground[ok]).all() and (a.ground[ok] <= a.ground_max[ok]).all()
    assert (a.ground[~ok] == a.fallback_z).all() and (a.ground_pixels[ok] >= a.min_ground).all()
    bmap = BY_NAME[name]["bmap"]
    ring = (bmap < 0) & (a.owner >= 0)
    assert a.n_ring_pixels == int(ring.sum()) and (a.low[~ring] == brute.INT32_MAX).all()
    assert ((a.dist > 0) == ring).all() and (a.owner[bmap >= 0] == bmap[bmap >= 0]).all()


def test_the_ring_is_the_l1_voronoi_diagram():
    """What the rounds compute, and why `corridor` cannot show what one would first ask of it: a ring pixel, reached round a
    corner, whose dist is greater than its L1 distance to its owner.  There is none on any map: let P be labelled c in round
    r, C the pixel of c nearest to P in L1, d their distance; r >= d.  Walk a monotone path from C to P.  If a building
    pixel other than C lies on it, the last such pixel X belongs to another building (a pixel of c would be nearer than C),
    only outside pixels lie between X and P, and the rounds label every one of them, P too, by round L1(X, P) < d <= r: P
    would not be free in round r.  So the path is free and P is labelled by round d.  Hence dist == L1 distance to the
    owner == L1 distance to the nearest building, and by induction along the same path the owner is the lowest index among
    the nearest.  Asserted here on every case and on random maps; test_cases_are_what_they_are_for asserts for `corridor`
    what its shape can show."""
    maps = [(c["bmap"], c["ring"]) for c in cases.CASES if c["n_buildings"]]
    rng = np.random.default_rng(7)
    for k in range(40):
        m = np.full((14, 17), -1, np.int32)
        for c in range(int(rng.integers(1, 6))):
            x, y = int(rng.integers(0, 15)), int(rng.integers(0, 12))
            m[y:y + int(rng.integers(1, 5)), x:x + int(rng.integers(1, 7))] = c
        if (m >= 0).any():
            maps.append((m, int(rng.integers(1, 9))))
    for m, ring in maps:
        owner, dist, ringimg, _ = tref.ring_rounds(m, ring)
        sel = ringimg >= 0
        assert np.array_equal(brute.l1_to_owner(m, owner)[sel], dist[sel].astype(np.int64))
        h, w = m.shape
        by, bx = np.nonzero(m >= 0)
        yy, xx = np.mgrid[0:h, 0:w]
        d = np.abs(yy[..., None] - by) + np.abs(xx[..., None] - bx)  # [h][w][building pixels]
        dmin = d.min(-1)
        lowest = np.where(d == dmin[..., None], m[by, bx], np.iinfo(np.int32).max).min(-1)
        want = np.where((m < 0) & (dmin <= ring), lowest, -1)
        assert np.array_equal(want, ringimg)


def test_cases_are_what_they_are_for():
    """every premise of the case table"""
    t = {}
    brute.terrain(*cases.args(BY_NAME["two_close"]), trace=t)
    a = ref("two_close")[0]
    assert t["contested"] >= 1 and (a.owner[8:16, 17] == 0).all() and (a.dist[8:16, 17] == 2).all()  # both reach column 17 in round 2
    # corridor: the pocket is sealed by the L and the image's corner, it is reached from the L alone, and (what "around a
    # corner" can mean: see test_the_ring_is_the_l1_voronoi_diagram) some ring pixel sees no pixel of its owner along its row
    # or its column within its dist
    c = BY_NAME["corridor"]
    a, m = ref("corridor")[0], c["bmap"]
    pocket = np.zeros(m.shape, bool)
    pocket[0:19, 30:40] = True
    assert (m[pocket] == -1).all() and (m[19, 30:40] == 1).all() and (m[0:19, 29] == 1).all()
    near = pocket & (a.dist > 0)
    assert near.any() and (a.owner[near] == 1).all() and (a.owner[pocket & ~near] == -1).all()
    turned = 0
    for y, x in np.argwhere((m < 0) & (a.owner >= 0)).tolist():
        o, d = a.owner[y, x], int(a.dist[y, x])
        turned += not ((m[y, max(x - d, 0):x + d + 1] == o).any() or (m[max(y - d, 0):y + d + 1, x] == o).any())
    assert turned >= 1
    a = ref("border")[0]
    assert a.ring_pixels[0] < 4 * 5 * 7 and a.owner[0, 6] == 0 and a.n_fallback == 0
    a = ref("outlier")[0]
    assert a.ground_min[0] == -5000 and a.ground[0] != a.ground_min[0] and abs(int(a.ground[0])) <= 5
    a = ref("empty_ring")[0]
    assert a.status.tolist() == [0, 1] and a.ground[1] == -777 and a.ground_pixels[1] == 0 and a.ring_pixels[1] > 0
    assert a.ground_min[1] == brute.INT32_MAX and a.ground_max[1] == brute.INT32_MIN
    a = ref("min_ground")[0]
    assert a.ground_pixels.tolist() == [cases.MIN_GROUND, cases.MIN_GROUND - 1] and a.status.tolist() == [0, 1] and a.ground[1] == -5
    for qn, qd in cases.RANK_Q:
        a = ref(f"ranks_{qn}_{qd}")[0]
        assert a.ground_pixels.tolist() == [1, 2, 5, 6] and a.n_fallback == 0
        assert a.ground.tolist() == [lows[(len(lows) - 1) * qn // qd] for lows in cases.RANK_LOWS]
        assert a.ring_points.tolist() == [2, 3, 6, 7]  # (the second point of one pixel counts as a point, not as a low)
    assert len({tuple(ref(f"ranks_{qn}_{qd}")[0].ground.tolist()) for qn, qd in cases.RANK_Q}) == 4
    a = ref("negative")[0]
    assert a.ground_min[0] < 0 < a.ground_max[0] and (a.low[a.low != brute.INT32_MAX] < 0).any()
    a, t = ref("many")
    assert a.n_buildings > tref.FIG_CAP and t["lds_buildings"] == tref.FIG_CAP and t["atomic_buildings"] == a.n_buildings - tref.FIG_CAP
    assert a.n_fallback == 0 and len(set(a.ground.tolist())) > 10
    a = ref("none")[0]
    assert a.n_buildings == 0 and a.n_ring_pixels == 0 and (a.owner == -1).all() and len(a.ground) == 0
    a = ref("early")[0]
    assert a.ring == brute.MAX_RING and 0 < a.rounds_used < a.ring and (a.owner >= 0).all()
    a = ref("slope")[0]
    g = a.ground.tolist()
    assert a.n_fallback == 0 and g[0] < g[1] < g[2] and g[1] - g[0] > 1000 and g[2] - g[1] > 1000


def test_the_big_run_takes_a_second_point_per_thread():
    c, a, t = big()
    assert a.grid * 256 < a.n_points < 2 * a.grid * 256 and t["second_point_threads"] > 0 and a.n_ring_points > a.grid * 64


def test_ranges_and_arguments_of_the_definition():
    """both references refuse what the definition refuses"""
    c = BY_NAME["two_close"]
    h, w = c["bmap"].shape

    def both(exc, **kw):
        a = dict(c, **kw)
        for f in (tref.terrain, brute.terrain):
            with pytest.raises(exc):
                f(*cases.args(a))

    def moved(col, v):
        x = c["xyz"].copy()
        x[3, col] = v
        return x

    both(brute.InvalidError, xyz=c["xyz"][:0])
    both(brute.InvalidError, bin=0)
    both(brute.InvalidError, n_buildings=-1)
    both(brute.InvalidError, ring=0)
    both(brute.InvalidError, ring=256)
    both(brute.InvalidError, q=(2, 1))
    both(brute.InvalidError, q=(-1, 1))
    both(brute.InvalidError, q=(0, 0))
    both(brute.InvalidError, min_ground=0)
    both(brute.RangeError, n_buildings=1)
    both(brute.RangeError, xyz=moved(0, -1))
    both(brute.RangeError, xyz=moved(1, -1))
    both(brute.RangeError, xyz=moved(0, w * c["bin"]))
    both(brute.RangeError, xyz=moved(1, h * c["bin"]))
    both(brute.RangeError, xyz=moved(2, 1 << 23))
    both(brute.RangeError, xyz=moved(2, -(1 << 23)))
    ok = dict(c, xyz=moved(2, (1 << 23) - 1))  # the largest height is inside
    assert brute.same(tref.terrain(*cases.args(ok)), brute.terrain(*cases.args(ok))) is None


def scene_maps(oracle):
    """name -> (cloud, building map of tests/building_ref on the footprint mask of the cloud's own raster, n_buildings,
    ground_th)"""
    sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
    sys.path.insert(0, os.path.join(HERE, "building_ref"))
    import building_ref as bref
    import ref as fref
    from test_roofs_cpu import load_roof_scenes
    out = {}
    for name, xyz in (("gabled", load_roof_scenes().gabled()), ("slope", cases.slope_scene())):
        img, th = oracle.grid_picture(xyz)
        _, mask = fref.footprints(img)
        b = bref.building_map(mask)
        out[name] = (xyz, b.map, b.n_buildings, th)
    return out


def test_end_to_end_premises_on_the_cpu(oracle):
    """what the device's end-to-end test builds on, with the map of tests/building_ref: three buildings each, no fallback
    at the defaults of Context.terrain, every ground of the gabled scene below 300 mm while ground_th is 3000, the grounds of
    the slope scene more than a metre apart"""
    sc = scene_maps(oracle)
    xyz, bmap, nb, th = sc["gabled"]
    t = tref.terrain(xyz, 100, bmap, nb, 10, (1, 2), 8, int(th))
    assert nb == 3 and th == 3000 and t.n_fallback == 0 and (t.ground < 300).all()
    xyz, bmap, nb, th = sc["slope"]
    t = tref.terrain(xyz, 100, bmap, nb, 10, (1, 2), 8, int(th))
    g = np.sort(t.ground)
    assert nb == 3 and t.n_fallback == 0 and (np.diff(g) > 1000).all()
