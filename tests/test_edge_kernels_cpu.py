"""The edge kernels without a GPU: the numpy restatements of tests/edge_ref/edge_ref.py against the reference reader's own
output (tests/golden/ply_edge_cases.npz) and against loops over the definitions, the premises of every case of
tests/edge_ref/cases.py (the truncation regimes, where the extremes sit, which owners and missing indices occur, how many
hook / MIN rounds the two-rank graphs need), and reach: every boundary has a case on each side.  tests/test_gpu_edge_kernels.py
then asks the device for the same cases."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_gpu_ingest import parse_binary  # noqa: E402


def load_edge_cases():
    if "edge_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("edge_cases", os.path.join(HERE, "edge_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["edge_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["edge_cases"]


cases = load_edge_cases()
ref = cases.ref
EDGE = np.load(os.path.join(HERE, "golden", "ply_edge_cases.npz"))


def fixture_file(name):
    """(body bytes, n, stride, offsets, is_f64, the reference reader's positions) of a file of the fixture"""
    buf = EDGE[name + "/in"].tobytes()
    n, stride, pos, kind, end = parse_binary(buf)
    return buf[end:end + n * stride], n, stride, (pos["x"], pos["y"], pos["z"]), kind["x"] == "float64", EDGE[name + "/xyz"]


def numpy_hook(rows, gidx, parent):
    """the numpy hook of tests/test_dist_gloo.py on numpy arrays (parent updated in place)"""
    import torch
    from test_dist_gloo import OracleBackend
    return OracleBackend.cc_hook(None, torch.from_numpy(rows), torch.from_numpy(gidx), torch.from_numpy(parent))


# ---- restatement against the reference's reader ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f[0] for f in cases.PLY_EDGE_FILES])
def test_ingest_restatement_equals_the_reference_reader(name):
    body, n, stride, off, is_f64, want = fixture_file(name)
    assert cases.ply_edge_file(name) == EDGE[name + "/in"].tobytes()  # the fixture is of the cases as they are now
    assert n == len(want) == len(cases.PLY_SWEEP) and is_f64 == dict((f[0], f[1]) for f in cases.PLY_EDGE_FILES)[name]
    assert any(o % 2 for o in off) and stride % 2  # packed records: coordinates at odd offsets
    xyz, bad = ref.ingest(body, n, stride, off, is_f64, cases.PLY_SCALE)
    assert not bad and xyz.dtype == np.int32
    assert np.array_equal(xyz, want)


def test_truncation_regimes_of_the_sweep():
    k = cases.PLY_SWEEP
    got = {}
    for name, _, _ in cases.PLY_EDGE_FILES:
        body, n, stride, off, is_f64, want = fixture_file(name)
        got[is_f64] = want[:, 0].astype(np.int64)
        v = ref.field(body, n, stride, off[0], is_f64)
        assert np.array_equal(v, (k / 1000.0).astype(np.float64 if is_f64 else np.float32).astype(np.float64))
    p64 = (k / 1000.0) * 1000.0
    assert int((got[True] != k).sum()) == cases.SWEEP_F64_TRUNC_NOT_K == 96
    assert int((np.trunc(p64) != np.floor(p64)).sum()) == cases.SWEEP_F64_TRUNC_NOT_FLOOR == 82
    assert int((got[True] != np.floor(p64)).sum()) == 82  # the reader truncates: flooring would move 82 of its values
    f32 = (k / 1000.0).astype(np.float32)
    assert int((got[False] != k).sum()) == cases.SWEEP_F32_TRUNC_NOT_K == 4946
    narrow = np.trunc((f32 * np.float32(1000.0)).astype(np.float64))
    assert int(((got[False] != k) & (narrow != got[False])).sum()) == cases.SWEEP_F32_PRODUCT_DIFFERS == 4856


@pytest.mark.parametrize("name", [f[0] for f in cases.PLY_EDGE_FILES])
def test_every_kind_of_value_is_in_the_fixture(name):
    body, n, stride, off, is_f64, want = fixture_file(name)
    dt = np.float64 if is_f64 else np.float32
    special = cases.ply_special_values(is_f64)
    assert {k for k, _ in special} == {"neg_fraction", "zero", "subnormal", "ulp_below", "ulp_at", "ulp_above", "largest"}
    assert len(special) <= n
    for axis in (1, 2):  # every special value is on y and on z, bit for bit
        have = set(ref.field(body, n, stride, off[axis], is_f64).astype(dt).view(np.int64 if is_f64 else np.int32).tolist())
        assert {int(np.array(v, dt).view(np.int64 if is_f64 else np.int32)) for _, v in special} <= have
    val = np.array([v for _, v in special], dt).astype(np.float64)
    kind = np.array([k for k, _ in special])
    prod = val * cases.PLY_SCALE
    assert (np.abs(prod) < 2147483649.0).all() and ((prod > ref.LO) & (prod < ref.HI)).all()  # nothing undefined in the file
    frac = prod[kind == "neg_fraction"]
    assert (frac < 0).all() and (np.trunc(frac) != np.floor(frac)).all()
    assert np.signbit(val[kind == "zero"]).tolist() == [False, True]
    sub = val[kind == "subnormal"]
    assert (np.abs(sub) < np.finfo(dt).tiny).all() and (sub != 0).all() and (np.trunc(sub * cases.PLY_SCALE) == 0).all()
    below, at, above = (np.trunc(prod[kind == k]) for k in ("ulp_below", "ulp_at", "ulp_above"))
    assert (below <= at).all() and (at <= above).all() and (below < above).any()
    assert (below < at).any() and (at < above).any()  # an ulp moves the truncated millimetre on either side
    big = prod[kind == "largest"]
    assert big[0] > 2147483000.0 and big[1] < -2147483000.0
    for v, s in zip(val[kind == "largest"], (1, -1)):  # the next value of the type no longer fits
        nxt = np.float64(np.nextafter(dt(v), dt(s * np.inf))) * cases.PLY_SCALE
        assert not (ref.LO < nxt < ref.HI)


# ---- restatements against loops over the definitions -------------------------------------------------------------------------
def test_restatements_against_loops():
    rng = np.random.default_rng(1)
    # ingest: struct.unpack per field
    import struct
    for s, o, f, off in cases.ingest_layouts():
        rec = cases.ingest_records(rng, 9, s, off, f, -1000.0)
        xyz, bad = ref.ingest(rec, 9, s, off, f, -1000.0)
        raw = rec.tobytes()
        for i in range(9):
            for a in range(3):
                v = struct.unpack_from("<d" if f else "<f", raw, i * s + off[a])[0] * -1000.0
                assert xyz[i, a] == int(v)  # (Python's int() truncates toward zero)
        assert not bad
    # the ends of the range and what lies beyond them
    for v, dt, want in cases.INGEST_ENDS:
        xyz, bad = ref.ingest(np.array([v, 0, 0], dt).tobytes(), 1, 3 * int(dt[2]), (0, int(dt[2]), 2 * int(dt[2])), dt == "<f8", 1.0)
        assert not bad and xyz[0, 0] == want
    for dt, vals in cases.INGEST_REJECTED.items():
        for v in vals:
            w = int(dt[2])
            assert ref.ingest(np.array([0, 0, v], dt).tobytes(), 1, 3 * w, (0, w, 2 * w), dt == "<f8", 1.0)[1]
    # tiles
    xyz, off = cases.tile_batch("mixed")
    box = ref.tile_boxes(xyz, off)
    sh, mn = ref.shift_tiles(xyz, off)
    for t in range(len(off) - 1):
        part = xyz[off[t]:off[t + 1]].astype(object)
        assert box[t].tolist() == [min(part[:, a]) for a in range(3)] + [max(part[:, a]) for a in range(3)]
        assert np.array_equal(sh[off[t]:off[t + 1]], xyz[off[t]:off[t + 1]].astype(np.int64) - box[t, :3]) and np.array_equal(mn[t], box[t, :3])
    assert np.array_equal(ref.shift_tiles(xyz, [0, len(xyz)])[0], ref.shift(xyz)[0])
    # labels, remap
    own, seeds, _ = cases.label_case(1000)
    assert ref.labels_from_owner(own, seeds).tolist() == [-1 if o < 0 else 1 + sum(1 for s in seeds.tolist() if s < o) for o in own.tolist()]
    assert ref.labels_from_owner(own, seeds[:0]).tolist() == [-1 if o < 0 else 1 for o in own.tolist()]
    c = cases.fuzz_case("remap", 3)
    out, miss = ref.remap(c["rows"], c["sg"])
    where = {int(g): i for i, g in enumerate(c["sg"].tolist())}
    assert out.reshape(-1).tolist() == [where.get(int(g), 0) for g in c["rows"].reshape(-1).tolist()]
    assert miss == any(int(g) not in where for g in c["rows"].reshape(-1).tolist())
    assert ref.remap(np.zeros((2, 3), np.int32), np.zeros(0, np.int32))[1] and not ref.remap(np.zeros((0, 3), np.int32), c["sg"])[1]
    # components: a union-find in plain Python
    c = cases.fuzz_case("hook", 5)
    par = list(range(c["n_total"]))

    def find(x):
        while par[x] != x:
            x = par[x]
        return x
    for u, row in zip(c["gidx"].tolist(), c["rows"].tolist()):
        for v in row:
            a, b = find(u), find(v)
            par[max(a, b)] = min(a, b)
    assert ref.components(c["n_total"], c["gidx"], c["rows"]).tolist() == [find(x) for x in range(c["n_total"])]
    # colours
    col = ref.colours(7, [[1, 2], [], [6]], [[1, 2, 3], [4, 5, 6], [65535, 0, 9]])
    assert col.dtype == np.uint16 and col.tolist() == [[0] * 3, [1, 2, 3], [1, 2, 3], [0] * 3, [0] * 3, [0] * 3, [65535, 0, 9]]


# ---- premises of the cases -------------------------------------------------------------------------------------------------
def test_ingest_cases_premises():
    lay = cases.ingest_layouts()
    assert {s for s, _, _, _ in lay} == set(cases.INGEST_STRIDES) and {o for _, o, _, _ in lay} == set(cases.INGEST_ORDERS)
    assert {(s, f) for s, _, f, _ in lay} == {(12, False), (15, False), (24, False), (24, True), (27, False), (27, True), (40, False), (40, True)}
    assert all(o[0] % 2 == 1 for _, order, _, o in lay if order == "rgb_first")
    rng = np.random.default_rng(2)
    for scale in cases.INGEST_SCALES:
        for f in (False, True):
            off = cases.ingest_offsets(27, "rgb_first", f)
            rec = cases.ingest_records(rng, 4097, 27, off, f, scale)
            xyz, bad = ref.ingest(rec, 4097, 27, off, f, scale)
            v = ref.field(rec, 4097, 27, off[0], f) * scale
            assert not bad and int(xyz.max()) - int(xyz.min()) < (1 << 31)  # the shift's contract
            assert ((v < 0) & (v != np.trunc(v))).any() and ((v > 0) & (v != np.trunc(v))).any() and (v == np.trunc(v)).any()
            assert (np.abs(v) < 1).any()
    n, at = cases.INGEST_REJECT_N, cases.INGEST_REJECT_AT
    assert n % cases.WG and n > cases.WG and at[0] == (0, 0) and at[1][0] == n - 1 and at[2][1] == 2 and 0 < at[2][0] < n - 1
    assert np.float32(cases.INGEST_ENDS[2][0]) == cases.INGEST_ENDS[2][0] == 2147483520.0
    assert all(np.float32(v) == v or v != v for v in cases.INGEST_REJECTED["<f4"])  # every float32 case is a float32


@pytest.mark.parametrize("n", cases.SHIFT_N)
def test_shift_cases_premises(n):
    seen = set()
    for place in cases.SHIFT_PLACES:
        xyz = cases.shift_cloud(n, place).astype(np.int64)
        idx = cases.shift_min_indices(n, place)
        for a in range(3):
            assert np.flatnonzero(xyz[:, a] == xyz[:, a].min()).tolist() == [idx[a]]  # the minimum is unique and sits there
        assert int(xyz.max()) - int(xyz.min()) < (1 << 31)
        seen.add(idx)
        if place == "lanes" and n > cases.WAVE:
            assert len({i % cases.WAVE for i in idx}) == 3 and len({i // cases.WG for i in idx}) == 3
            if n > cases.MINMAX_TRIP:
                assert sum(i >= cases.MINMAX_TRIP for i in idx) >= (2 if n > cases.MINMAX_TRIP + 6 * cases.WG else 1)  # only the second trip reads them
        if place == "last" and n > cases.MINMAX_TRIP:
            assert idx[0] >= cases.MINMAX_TRIP
    assert len(seen) == (3 if n > 1 else 1)


def test_shift_further_clouds_premises():
    by = dict(cases.shift_further_clouds())
    assert (by["equal"] == by["equal"][0]).all() and (by["negative"] < 0).all()
    w = by["widest"].astype(np.int64)
    assert (w.min(0) == cases.I32_MIN).all() and (w.max(0) - w.min(0) == (1 << 31) - 1).all()


def test_tile_cases_premises():
    C = cases.TILE_CHUNK
    assert cases.TILE_BATCHES["mixed"] == (1, C - 1, C, C + 1, 2 * C + 1, 1, 1, 3 * C + 1)
    assert cases.TILE_BATCHES["thousand_points"] == (1,) * 1000 and len(cases.TILE_BATCHES["one_tile"]) == 1
    xyz, off = cases.tile_batch("mixed")
    used = set()
    for t, ln in enumerate(np.diff(off)):
        part = xyz[off[t]:off[t + 1]].astype(np.int64)
        places = cases.tile_extreme_places(ln)
        for a in range(3):
            lo, hi = int(part[:, a].argmin()), int(part[:, a].argmax())
            assert lo in places and hi in places
            if ln > C:
                used.update((lo, hi) if ln - 1 not in (lo, hi) else ())
                used.update({"first" for i in (lo, hi) if i == 0} | {"last" for i in (lo, hi) if i == ln - 1})
    assert {C - 1, C, "first", "last"} <= used  # extremes either side of a chunk boundary, at the first and at the last point


def test_label_cases_premises():
    for ns in cases.LABEL_N_SEEDS:
        own, seeds, kinds = cases.label_case(ns)
        assert len(seeds) == ns and (np.diff(seeds) > 0).all()
        want = {"minus1", "minus2", "negative"} | ({"seed", "between", "below", "above"} if ns > 1 else {"seed", "below", "above"} if ns else {"no_seeds"})
        assert set(kinds.tolist()) == want
        o = own.astype(np.int64)
        assert np.isin(o[kinds == "seed"], seeds).all() and len(np.unique(o[kinds == "seed"])) == ns
        assert not np.isin(o[kinds == "between"], seeds).any()
        if ns:
            assert (o[kinds == "below"] < seeds[0]).all() and (o[kinds == "above"] > seeds[-1]).all()
            b = o[kinds == "between"]
            assert ((b > seeds[0]) & (b < seeds[-1])).all()
        lab = ref.labels_from_owner(own, seeds)
        assert (lab[o < 0] == -1).all() and lab[o >= 0].min() == 1 and lab.max() == ns + 1


def test_scene_has_owners_that_are_no_committed_seeds(oracle):
    """what tests/test_gpu_shard.py and test_gpu_edge_kernels.py take from synth.boxes(): labelled points whose owner is an
    attempt that did not commit, owners below the first committed seed and above the last one"""
    from buildingsegment_amd import synth
    xyz = synth.boxes()
    ng, nr = oracle.knn_normals(xyz, k=15)
    pi, pl, ow = oracle.region_grow(xyz, nr, ng, want_owner=True)
    seeds = pl["point_idx"][pl["offset"][:-1]]
    lab = ow >= 0
    assert np.array_equal(lab, pi > 0) and len(seeds) >= 2
    assert (~np.isin(ow[lab], seeds)).any() and (ow[lab] < seeds.min()).any() and (ow[lab] > seeds.max()).any()
    assert np.array_equal(ref.labels_from_owner(ow, seeds), np.where(lab, pi, -1))


def test_colour_cases_premises():
    sizes = []
    for name in cases.COLOUR_CLOUDS:
        g = np.load(os.path.join(HERE, "golden", name + ".npz"))
        assert len(g["xyz"]) <= 12_000
        sizes += np.diff(g["offset"]).tolist()
    assert max(sizes) > cases.COLOUR_BIG_PLANE >= 16 * cases.WG and min(sizes) < cases.COLOUR_BIG_PLANE
    rgb = cases.colour_table(5)
    assert rgb.min() == 0 and rgb.max() == 65535


def test_remap_cases_premises():
    T = cases.REMAP_TABLE
    for k in cases.REMAP_K:
        lo, hi = cases.REMAP_ROWS[k]
        assert lo * k < T <= hi * k and T - lo * k <= k and hi * k - T < k  # the nearest row counts either side
    assert cases.REMAP_ROWS[1] == (T - 1, T) and cases.REMAP_ROWS[3][0] * 3 == T - 1 and cases.REMAP_ROWS[16][1] * 16 == T
    flat, sg = cases.remap_input()
    assert len(flat) >= max(r * k for k in cases.REMAP_K for r in cases.REMAP_ROWS[k])
    assert (np.diff(sg) > 0).all() and sg[0] >= 0 and sg[-1] < (1 << 24) and np.isin(flat[:100_000], sg).all()
    miss = cases.remap_missing(sg)
    assert set(miss) == {"negative", "last_plus_1", "far_above", "inside_absent"}
    assert all(v < 0 for v in miss["negative"]) and miss["last_plus_1"] == (int(sg[-1]) + 1,)
    assert all(v > sg[-1] + 1 for v in miss["far_above"]) and all(sg[0] < v < sg[-1] for v in miss["inside_absent"])
    assert not np.isin(np.concatenate([np.array(v, np.int64) for v in miss.values()]), sg).any()


@pytest.mark.parametrize("k", cases.HOOK_K)
def test_hook_cases_premises(k):
    for permuted in (False, True):
        gidx, rows = cases.hook_case(k, permuted)
        n = cases.HOOK_N_TOTAL
        assert len(gidx) == n // 3 and len(np.unique(gidx)) == len(gidx) and rows.shape == (len(gidx), k)
        assert rows.min() >= 0 and rows.max() < n and gidx.min() >= 0 and gidx.max() < n  # the library does not check this
        assert (np.diff(gidx) > 0).all() != permuted
        assert (rows[:, 0] != gidx).any() and (rows[:, 0] == gidx).any()  # slot 0 is another point, and the point itself
        assert (rows == gidx[:, None]).any()  # self loops
        if k > 1:
            assert (rows[:, 0] == rows[:, 1]).any() and (rows[:, k - 1] == gidx).any()
            # edges that only the last slot carries, between components the other slots leave apart
            without = ref.components(n, gidx, rows[:, :k - 1])
            assert (without != ref.components(n, gidx, rows)).any()
        parent = ref.components(n, gidx, rows)
        ncomp = int((parent == np.arange(n)).sum())
        sizes = np.bincount(parent)
        assert (parent <= np.arange(n)).all() and 100 < ncomp < n - 100 and sizes.max() > 8 and (sizes == 1).any()


@pytest.mark.parametrize("graph", cases.HOOK_GRAPHS)
@pytest.mark.parametrize("ranks", cases.HOOK_RANKS)
def test_hook_rounds_of_the_rank_graphs(graph, ranks):
    n, order, rows = cases.hook_graph(graph)
    assert n <= 2048 and rows.min() >= 0 and rows.max() < n and sorted(order.tolist()) == list(range(n))
    want = ref.components(n, order, rows)
    assert (want == 0).all()  # one component
    deal = cases.hook_deal(order, rows, ranks)
    assert sum(len(g) for g, _ in deal) == n
    parent, rounds, per_round = cases.hook_rounds(n, deal, numpy_hook)
    assert np.array_equal(parent, want)
    assert 3 <= rounds <= n // 16, per_round  # several rounds, and far inside the cap of n
    assert per_round[-1] == 0 and all(h > 0 for h in per_round[:-1])
    # one rank with every row needs one hooking round
    assert cases.hook_rounds(n, cases.hook_deal(order, rows, 1), numpy_hook)[1] == 2


# ---- fuzz and reach ----------------------------------------------------------------------------------------------------------
def test_fuzz_cases_reach_the_boundaries():
    C = [[cases.fuzz_case(e, s) for s in range(cases.FUZZ_CASES)] for e in cases.FUZZ_ENTRIES]
    by = dict(zip(cases.FUZZ_ENTRIES, C))
    n = [c["n"] for c in by["ingest"]]
    assert min(n) <= cases.WAVE < cases.WG < max(n) and {c["is_f64"] for c in by["ingest"]} == {False, True}
    assert {c["lead"] % 4 for c in by["ingest"]} == {0, 1, 2, 3} and len({c["stride"] for c in by["ingest"]}) == 5
    assert all(not ref.ingest(c["records"], c["n"], c["stride"], c["off"], c["is_f64"], c["scale"])[1] for c in by["ingest"])
    n = [c["n"] for c in by["shift"]]
    assert min(n) <= cases.WG and sum(x > cases.MINMAX_TRIP for x in n) >= 3 and sum(cases.WG < x <= cases.MINMAX_TRIP for x in n) >= 3
    assert all(int(c["xyz"].astype(np.int64).max()) - int(c["xyz"].astype(np.int64).min()) < (1 << 31) for c in by["shift"])
    lens = np.concatenate([np.diff(c["off"]) for c in by["tiles"]])
    assert (lens >= 1).all() and (lens == 1).any() and (lens < cases.TILE_CHUNK).any() and (lens > cases.TILE_CHUNK).any() and (lens > 2 * cases.TILE_CHUNK).any()
    assert {len(c["off"]) - 1 for c in by["tiles"]} >= {1, 2, 300}
    assert all((cc["xyz"].astype(np.int64).max(0) - cc["xyz"].astype(np.int64).min(0) < (1 << 31)).all() for cc in by["tiles"])
    assert {len(c["seeds"]) for c in by["labels"]} >= {0, 1, 256, 1000}
    assert any(ref.remap(c["rows"], c["sg"])[1] for c in by["remap"]) and any(not ref.remap(c["rows"][:0], c["sg"])[1] for c in by["remap"])
    assert {c["k"] for c in by["hook"]} >= {1, 4, 5, 64}
    assert all(c["rows"].min() >= 0 and c["rows"].max() < c["n_total"] and c["gidx"].max() < c["n_total"] for c in by["hook"])


def test_every_boundary_has_a_case_on_each_side():
    B = cases.boundaries()
    assert len(B) >= 16
    for name, (b, lo, hi) in B.items():
        assert lo and hi, name
    # the sizes the directed tests use are the nearest ones on either side
    for name in ("ingest: records of a wave (64)", "ingest: records of a workgroup (256)", "shift: points of one grid-stride trip (131072)",
                 "tiles: points of a chunk (4096)", "labels: owners of a workgroup (256)", "hook: k fills 1 quad(s) (4)", "hook: the largest k (64)"):
        b, lo, hi = B[name]
        assert b - max(lo) <= 1 and min(hi) - b <= 1 and max(lo) < min(hi), name
    assert set(cases.SHIFT_N) >= {cases.MINMAX_TRIP - 1, cases.MINMAX_TRIP, cases.MINMAX_TRIP + 1}
    assert set(cases.INGEST_N) >= {63, 64, 65, 255, 256, 257, 4097}
    assert set(cases.HOOK_K) == {1, 2, 3, 4, 5, 7, 8, 15, 16, 63, 64} and set(cases.REMAP_K) == {1, 3, 16}
    assert set(cases.LABEL_N_SEEDS) == {0, 1, 2, 1000, 100_000}
