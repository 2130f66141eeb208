"""Polygon solids without a GPU (include/bs_api.h, "polygon solids"): the numpy restatement of the device algorithm against
the brute force of the definition on every run of the cases, and the two promises checked without the algorithm, with Python
integers: per closed building every directed edge occurs as often as its reverse, and the determinants of the fan triangles
of all its faces add up to volume6."""
import importlib.util
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_triangulate_cpu import RUNS as TRI_RUNS, ref as tri_ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_poly_solids_count_dev", "bs_poly_solids_emit_dev", "bs_poly_solids", "bs_poly_solids_free"]


def load_polysolid_cases():
    if "polysolid_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("polysolid_cases", os.path.join(HERE, "polysolid_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["polysolid_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["polysolid_cases"]


cases = load_polysolid_cases()
pref, brute, tref, tbrute, uref = cases.pref, cases.brute, cases.tref, cases.tbrute, cases.uref
OWN = cases.own_shapes()
BY_NAME = {}
for _name, _c, _tol, _kind, _base in cases.all_runs():
    BY_NAME.setdefault(_name, (_c, []))[1].append((_tol, _kind, _base))
_UP, _REF = {}, {}


def upstream(name, tol):
    """(plain, clean, triangles) of the restatements of the stages before, computed once and never changed"""
    if name in TRI_RUNS and name not in OWN:
        return tri_ref(name, tol)
    if (name, tol) not in _UP:
        c = BY_NAME[name][0]
        plain, _, clean = uref.clean(c["label"], c["top"], c["n_labels"], *tol)
        _UP[name, tol] = (plain, clean, tref.triangulate(plain, clean))
    return _UP[name, tol]


def ref(name, tol, kind, base):
    """(the restatement's result, its trace, label_building, n_buildings), computed once and never changed"""
    key = (name, tol, kind, base)
    if key not in _REF:
        plain, clean, tri = upstream(name, tol)
        lb, nb = cases.table(kind, BY_NAME[name][0]["n_labels"])
        trace = {}
        _REF[key] = (pref.poly_solids(plain, clean, tri, lb, nb, cases.BIN, base, trace), trace, lb, nb)
    return _REF[key]


def check_promises(s, bin):
    """per closed building: every directed edge as often as its reverse; the fan determinants add up to volume6"""
    V = np.asarray(s.vertex, np.int64).tolist()
    off, idx, fb = s.face_offset.tolist(), s.face_index.tolist(), s.face_building.tolist()
    edges = [Counter() for _ in range(s.n_buildings)]
    det = [0] * s.n_buildings
    for f, c in enumerate(fb):
        p = idx[off[f]:off[f + 1]]
        assert len(p) >= 3 and all(V[v][3] == c for v in p)
        assert all(p[k] != p[(k + 1) % len(p)] for k in range(len(p)))
        for k in range(len(p)):
            edges[c][(p[k], p[(k + 1) % len(p)])] += 1
        x0, y0, z0 = V[p[0]][0] // bin, V[p[0]][1] // bin, V[p[0]][2]
        for k in range(1, len(p) - 1):
            x1, y1, z1 = V[p[k]][0] // bin, V[p[k]][1] // bin, V[p[k]][2]
            x2, y2, z2 = V[p[k + 1]][0] // bin, V[p[k + 1]][1] // bin, V[p[k + 1]][2]
            det[c] += x0 * (y1 * z2 - z1 * y2) - y0 * (x1 * z2 - z1 * x2) + z0 * (x1 * y2 - y1 * x2)
    for c in range(s.n_buildings):
        assert all(edges[c][(b, a)] == n for (a, b), n in edges[c].items()), c
        assert det[c] == int(s.volume6[c]), (c, det[c], int(s.volume6[c]))
        if s.status[c]:
            assert not edges[c] and s.vertices[c] == 0 and s.faces[c] == 0 and s.volume6[c] == 0
    assert all(v % bin == 0 for q in V for v in q[:2])
    assert V == sorted(V, key=lambda q: (q[3], q[1], q[0], q[2])) and len(set(map(tuple, V))) == len(V)


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert re.search(r"^struct bs_poly_solids \{", txt, flags=re.M)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("poly_solids", "poly_solids_dev", "poly_solids_emit_dev", "building_model"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "PolySolids") and L.bs_api_version() == 5
    cap, = re.findall(r"^#define BS_POLY_FIG_CAP (\d+)", txt, flags=re.M)
    assert int(cap) == _lib.POLY_FIG_CAP == pref.FIG_CAP
    # the struct of the loader follows the header field for field
    body = re.search(r"^struct bs_poly_solids \{(.*?)^\};", txt, flags=re.M | re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", decl.strip())]
    assert names == [f[0] for f in _lib.PolySolids._fields_]


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_references_agree_and_promises_hold(name):
    """on every run of the cases: the restatement equals the definition in every array and figure, and the mesh keeps both
    promises"""
    for tol, kind, base in BY_NAME[name][1]:
        a, _, lb, nb = ref(name, tol, kind, base)
        plain, clean, tri = upstream(name, tol)
        b = brute.poly_solids(plain, clean, tri, lb, nb, cases.BIN, base)
        assert brute.same(a, b) is None, (tol, kind, base, brute.same(a, b))
        check_promises(a, cases.BIN)


@pytest.mark.parametrize("name", ["nested", "two_outers", "random_0", "random_1", "random_2", "fuzz_0", "sieve_24"])
def test_volume_of_flat_roofs(name):
    """a top that is constant per label, every node kept: volume6 of a building is 6 * pixels * (t - base_z) over its labels"""
    c = BY_NAME[name][0]
    lab, nl = c["label"], c["n_labels"]
    t = 100 + 37 * np.arange(nl + 1, dtype=np.int64)
    top = np.repeat(t[lab][..., None], 4, axis=2).astype(np.int32)
    plain, _, clean = uref.clean(lab, top, nl, 0, 1)
    tri = tref.triangulate(plain, clean)
    for kind in cases.TABLES:
        for base in (-1000, 150):
            lb, nb = cases.table(kind, nl)
            s = pref.poly_solids(plain, clean, tri, lb, nb, cases.BIN, base)
            assert s.n_open_buildings == 0
            want = np.zeros(nb, np.int64)
            for l in range(nl):
                want[lb[l]] += 6 * int((lab == l).sum()) * (int(t[l]) - base)
            assert np.array_equal(s.volume6, want) and s.total_volume6 == want.sum()
            assert np.array_equal(s.area2, np.bincount(lb, [2 * (lab == l).sum() for l in range(nl)], nb).astype(np.int64))
            check_promises(s, cases.BIN)


def test_every_regime_is_reached():
    """the rows of the threshold table ("Polygon solids"), worked out from the case inputs"""
    reached = {}
    for name, (c, runs) in BY_NAME.items():
        if name.startswith(("fuzz_", "line_", "random_")) and name not in ("random_0", "fuzz_1"):
            continue  # (what they reach the shapes reach too: the refs of the rest are enough for this test)
        for tol, kind, base in runs:
            s, trace, lb, nb = ref(name, tol, kind, base)
            for r in cases.regimes(upstream(name, tol)[2], lb, nb, trace, s):
                reached.setdefault(r, (name, tol, kind, base))
    assert sorted(reached) == sorted(cases.REGIMES), sorted(set(cases.REGIMES) - set(reached))
    print(reached)


def test_shapes_are_what_they_are_for():
    def one(name, i=0):
        tol, kind, base = BY_NAME[name][1][i]
        return ref(name, tol, kind, base)[0]

    def walls(s):
        return [s.face_index[s.face_offset[f]:s.face_offset[f + 1]].tolist() for f in np.flatnonzero(s.face_kind == 2)]

    inner = lambda s: [w for w in walls(s) if len({tuple(s.vertex[v][:2]) for v in w}) == 2 and  # noqa: E731
                       {tuple(s.vertex[v][:2] // cases.BIN) for v in w} == {(1, 0), (1, 1)}]
    assert [len(w) for w in inner(one("wall_3"))] == [3] and [len(w) for w in inner(one("wall_4"))] == [4]
    assert inner(one("wall_flush")) == [] and one("wall_flush").n_wall_faces == 6
    assert [len(w) for w in inner(one("wall_between"))] == [6] == [len(w) for w in inner(one("wall_between_reversed"))]
    assert one("wall_crossing").n_crossing_walls == 1 and one("wall_crossing", 1).n_crossing_walls >= 1
    assert one("wall_8").max_wall_vertices_all == 8 and one("wall_8", 1).max_wall_vertices_all == 10
    other = one("wall_other_building")
    assert other.n_wall_faces == 8 and (other.wall_faces == 4).all() and other.n_buildings == 2
    assert (one("wall_below_base").z_max < 1000).all() and one("wall_below_base").total_volume6 < 0
    assert one("courtyard").n_wall_faces == 8
    z = lambda s, X, Y, c: sorted(int(v[2]) for v in s.vertex if tuple(v[:2] // cases.BIN) == (X, Y) and v[3] == c)  # noqa: E731
    assert z(one("corner_of_four"), 1, 1, 0) == [-1000, 10, 20, 30, 40]
    assert [z(one("corner_of_four", 1), 1, 1, c) for c in range(4)] == [[-1000, 10 + 10 * c] for c in range(4)]
    lw = one("label_without_ring")
    assert lw.labels.tolist() == [4] and lw.n_roof_faces == 4 and one("label_without_ring", 1).labels.tolist() == [2, 1, 1]
    e = one("no_label_pixel")
    assert (e.n_vertices, e.n_faces, e.n_indices) == (0, 0, 0) and e.face_offset.tolist() == [0] and e.labels.tolist() == [2]
    for n in (1023, 1024, 1025, 5000):
        s = one(f"strip_{n}")
        assert s.n_buildings == n and (s.vertices == 8).all() and (s.faces == 8).all() and s.n_open_buildings == 0
    (name, tol, l), = cases.tc.NO_BRIDGE_RUNS
    s, _, lb, nb = ref(name, tol, "mod3", -1000)
    assert s.status.tolist() == [1, 0, 0] and s.vertices[0] == 0 and s.faces[0] == 0 and not (s.face_building == 0).any()
    assert ref(name, tol, "one", 0)[0].n_faces == 0 and ref(name, tol, "one", 0)[0].n_open_buildings == 1


def test_obj_text_of_the_reference():
    s = ref("nested", (0, 1), "mod3", -1000)[0]
    lines = brute.obj_text(s, (1000, -2000, 30)).decode().split("\n")
    assert lines[0] == f"# solids: 3 buildings, {s.n_vertices} vertices, {s.n_faces} faces" and lines[-1] == ""
    assert sum(x.startswith("v ") for x in lines) == s.n_vertices and sum(x.startswith("f ") for x in lines) == s.n_faces
    assert [x for x in lines if x.startswith("o ")] == [f"o building_{c}" for c in range(3)]
