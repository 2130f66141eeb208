"""Simplified outlines without a GPU (include/bs_api.h, "simplified outlines"): the numpy restatement of the device
algorithm against the brute force that recurses per arc, the identities every result must satisfy, the regimes the device
suite's cases reach, simplify_tolerance, and the host-only writer bs_simple_outlines_write_obj against a file written by
hand."""
import ctypes as C
import importlib.util
import os
import re
import sys
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_simple_outlines_count_dev", "bs_simple_outlines_emit_dev", "bs_simple_outlines", "bs_simple_outlines_free",
       "bs_simple_outlines_write_obj"]


def load_simplify_cases():
    """tests/simplify_ref/cases.py under a name of its own (other reference directories have a cases.py too)"""
    if "simplify_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("simplify_cases", os.path.join(HERE, "simplify_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["simplify_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["simplify_cases"]


cases = load_simplify_cases()
sref, brute = cases.sref, cases.brute
NAMED = dict(cases.named_cases())
BIG = {name: (c, tols) for name, c, tols in cases.big_cases()}
_REF = {}


def ref(name, tol):
    """(plain, simplified) of the restatement, computed once per case and tolerance and never changed"""
    if (name, tol) not in _REF:
        c = NAMED[name] if name in NAMED else BIG[name][0]
        _REF[name, tol] = cases.run_ref(c, tol)
    return _REF[name, tol]


def tolerances(name):
    return cases.TOLERANCES if name in NAMED else BIG[name][1]


def ring_rows(plain, s, r):
    """the kept vertices of ring r as tuples (X, Y, Z, right, flag)"""
    a, b = int(s.s_ring_offset[r]), int(s.s_ring_offset[r + 1])
    z = s.sz if s.sz is not None else np.zeros(s.n_svertices, np.int32)
    return [(int(s.sxy[v, 0]), int(s.sxy[v, 1]), int(z[v]), int(s.s_right[v]), int(s.s_flag[v])) for v in range(a, b)]


def match_subsequence(small, big):
    """the positions in `big` of the rows of `small`, in order (greedy); None if small is no subsequence of big"""
    out, j = [], 0
    for row in small:
        while j < len(big) and big[j] != row:
            j += 1
        if j == len(big):
            return None
        out.append(j)
        j += 1
    return out


def twin_identity(plain, s):
    """every segment with s_right = B >= 0 occurs exactly once more, reversed, in a ring of B with the first ring's label
    as its s_right"""
    seen = Counter()
    for r in range(plain.n_rings):
        a, b = int(s.s_ring_offset[r]), int(s.s_ring_offset[r + 1])
        for v in range(a, b):
            u = v + 1 if v + 1 < b else a
            seen[int(plain.ring_label[r]), int(s.sxy[v, 0]), int(s.sxy[v, 1]), int(s.sxy[u, 0]), int(s.sxy[u, 1]),
                 int(s.s_right[v])] += 1
    for (lab, x0, y0, x1, y1, right), k in seen.items():
        if right >= 0:
            assert k == 1 and seen[right, x1, y1, x0, y0, lab] == 1, (lab, x0, y0, x1, y1, right)


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert re.search(r"^struct bs_simple_outlines \{", txt, flags=re.M)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("simplified_outlines", "simplified_outlines_dev", "simplified_outlines_emit_dev", "roof_polygons"):
        assert hasattr(api.Context, name), name
    for name in ("write_simple_outlines_obj", "SimpleOutlines", "simplify_tolerance"):
        assert hasattr(api, name), name
    s = _lib.SimpleOutlines()
    L.bs_simple_outlines_free(C.byref(s))  # a zeroed struct is accepted
    L.bs_simple_outlines_free(None)


@pytest.mark.parametrize("name", sorted(NAMED) + sorted(BIG))
def test_references_agree(name):
    c = NAMED[name] if name in NAMED else BIG[name][0]
    for tol in tolerances(name):
        plain, a = ref(name, tol)
        _, b = brute.simplify(c["label"], c["top"], c["n_labels"], *tol)
        assert sref.same(a, b) is None, (tol, sref.same(a, b))
        _, flat = sref.simplify(c["label"], None, c["n_labels"], *tol)  # without top: the same vertices, no sz
        assert flat.sz is None and np.array_equal(flat.sxy, a.sxy) and np.array_equal(flat.s_flag, a.s_flag)


@pytest.mark.parametrize("name", sorted(NAMED) + sorted(BIG))
def test_identities(name):
    tols = sorted(tolerances(name), key=lambda t: Fraction(*t))
    plain, nodes = ref(name, (0, 1))
    # with num = 0 exactly the nodes are kept, and the areas are the plain rings'
    assert nodes.n_svertices == nodes.n_nodes and np.array_equal(nodes.s_ring_area2, plain.ring_area2)
    assert np.array_equal(nodes.s_ring_arcs.sum(), nodes.n_arcs) and (nodes.s_flag & 1).sum() == nodes.n_junction_nodes
    node_rows = [ring_rows(plain, nodes, r) for r in range(plain.n_rings)]
    prev_rows = node_rows
    for num, den in tols:
        _, s = ref(name, (num, den))
        assert (s.n_rings, s.n_nodes, s.n_arcs) == (plain.n_rings, nodes.n_nodes, nodes.n_arcs)
        assert np.array_equal(np.diff(s.s_ring_offset), s.s_ring_vertices)
        rows = [ring_rows(plain, s, r) for r in range(plain.n_rings)]
        twin_identity(plain, s)
        for r in range(plain.n_rings):
            at = match_subsequence(rows[r], node_rows[r])
            assert at is not None, (num, den, r)  # the kept vertices are a subsequence of the ring's nodes
            assert match_subsequence(rows[r], prev_rows[r]) is not None, (num, den, r)  # ... and of a smaller tolerance's
            nn = len(node_rows[r])
            for j, a in enumerate(at):
                b = at[(j + 1) % len(at)]
                S, E = node_rows[r][a], node_rows[r][b]
                len2 = (E[0] - S[0]) ** 2 + (E[1] - S[1]) ** 2
                m = (a + 1) % nn
                while m != b:  # every dropped node against the kept segment that spans it
                    P = node_rows[r][m]
                    cr = (E[0] - S[0]) * (P[1] - S[1]) - (E[1] - S[1]) * (P[0] - S[0])
                    assert cr * cr * den <= num * len2, (num, den, r, S, P, E)
                    m = (m + 1) % nn
        prev_rows = rows


def test_every_ring_keeps_at_least_three_vertices():
    """A ring with exactly two junction nodes at different corners is two open arcs; the forced first split of every arc
    keeps a third vertex on the arc that has interior nodes (both cannot be straight).  `side_by_side` at (10^6, 1) is
    the smallest such case: either rectangle keeps the far corner with the lower corner index."""
    for name in sorted(NAMED) + sorted(BIG):
        for tol in tolerances(name):
            _, s = ref(name, tol)
            assert (s.s_ring_vertices >= 3).all(), (name, tol)
    _, s = ref("side_by_side", (10 ** 6, 1))
    assert s.sxy.tolist() == [[0, 0], [4, 0], [4, 6], [4, 0], [8, 0], [4, 6]]


def test_cases_reach_every_regime():
    """Every row of the threshold table of DESIGN.md ("Simplified outlines") is reached by the cases and tolerances of
    tests/test_gpu_simplify.py, worked out from the references."""
    seen = Counter()
    for name, c, tol in cases.all_runs():
        seen.update(cases.regimes(c, tol))
    missing = [k for k in cases.REGIMES if seen[k] == 0]
    assert not missing, missing
    t = {}
    cases.run_ref(BIG["thin_u_400"][0], (cases.BIG_DEN, cases.BIG_DEN), t)
    assert t["max_product"] >= 1 << 64


def test_expected_shapes():
    """results small enough to work out by hand"""
    _, s = ref("one_pixel", (10 ** 6, 1))
    assert s.sxy.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]] and s.s_flag.tolist() == [2, 0, 0, 0] and s.rounds == 1
    assert (s.n_nodes, s.n_junction_nodes, s.n_arcs, s.max_arc_nodes) == (4, 0, 1, 5)
    _, s = ref("rectangle", (10 ** 6, 1))
    assert s.sxy.tolist() == [[0, 0], [9, 0], [9, 5], [0, 5]] and s.s_ring_area2.tolist() == [90]
    plain, s = ref("side_by_side", (1, 1))  # two labels, junctions (4, 0) and (4, 6) on the image border
    assert s.s_ring_arcs.tolist() == [2, 2] and s.n_junction_nodes == 4
    assert s.sxy.tolist() == [[0, 0], [4, 0], [4, 6], [0, 6], [4, 0], [8, 0], [8, 6], [4, 6]]
    assert s.s_right.tolist() == [-1, 1, -1, -1, -1, -1, -1, 0]
    _, s = ref("junction_in_run", (0, 1))  # (2, 2) lies in the straight lower border of label 0: a node that is no vertex
    assert [2, 2] in s.sxy[:int(s.s_ring_offset[1])].tolist() and s.n_nodes == s.n_svertices
    _, s0 = ref("noisy_diagonal", (0, 1))
    _, s1 = ref("noisy_diagonal", (25, 4))
    assert s1.n_svertices < s0.n_svertices // 4 and s0.rounds >= 8


def test_simplify_tolerance():
    assert api.simplify_tolerance(0, 100) == (0, 1)
    assert api.simplify_tolerance(100, 100) == (1, 1)
    assert api.simplify_tolerance(50, 100) == (1, 4)
    assert api.simplify_tolerance(250, 100) == (25, 4)
    assert api.simplify_tolerance(30, 25) == (36, 25)
    assert api.simplify_tolerance(46340, 1) == (46340 ** 2, 1)
    for bad in ((-1, 100), (10, 0), (1.5, 100), (46341, 1)):
        with pytest.raises(ValueError):
            api.simplify_tolerance(*bad)


HAND_OBJ = b"""# simplified outlines: 2 labels, 3 rings, 12 vertices, tol2 1/4
g label_0_ring_0_outer
v 1000 -2000 100
v 1225 -2000 100
v 1225 -1775 100
v 1000 -1775 100
l 1 2 3 4 1
g label_0_ring_1_hole
v 1125 -1900 100
v 1100 -1900 100
v 1100 -1875 100
v 1125 -1875 100
l 5 6 7 8 5
g label_1_ring_0_outer
v 1100 -1900 100
v 1125 -1900 100
v 1125 -1875 100
v 1100 -1875 100
l 9 10 11 12 9
"""


def test_writer_against_a_file_written_by_hand(tmp_path):
    lab = np.zeros((9, 9), np.int32)
    lab[4, 4] = 1
    plain, s = sref.simplify(lab, np.full((9, 9, 4), 70, np.int32), 2, 1, 4)
    o = api.SimpleOutlines(9, 9, 2, 1, 4, s.n_rings, s.n_nodes, s.n_junction_nodes, s.n_arcs, s.n_svertices, s.rounds,
                           s.max_arc_nodes, plain.ring_label, plain.ring_area2, s.s_ring_vertices, s.s_ring_area2, s.s_ring_arcs,
                           s.s_ring_offset, plain.label_ring_offset, has_z=True, sxy=s.sxy, sz=s.sz, s_right=s.s_right,
                           s_flag=s.s_flag)
    api.write_simple_outlines_obj(o, tmp_path / "s.obj", 25, origin=(1000, -2000, 30))
    got = open(tmp_path / "s.obj", "rb").read()
    assert got == HAND_OBJ
    assert got == brute.obj_text(plain, s, 25, 1, 4, (1000, -2000, 30))
    o.sz = None  # without Z: 0 + origin
    api.write_simple_outlines_obj(o, tmp_path / "s.obj", 25, origin=(1000, -2000, 30))
    assert open(tmp_path / "s.obj", "rb").read() == HAND_OBJ.replace(b" 100\n", b" 30\n")
    L = _lib.load()
    assert L.bs_simple_outlines_write_obj(None, 25, None, str(tmp_path / "s.obj").encode()) == -1
    o.sxy = None
    with pytest.raises(ValueError):
        api.write_simple_outlines_obj(o, tmp_path / "s.obj", 25)
