"""Clean outlines without a GPU (include/bs_api.h, "clean outlines"): the numpy restatement of the device algorithm
against the brute force over all pairs, the properties every result must have -- checked by an all-pairs test of its own
with the parameters of the common point as integers -- and the regimes the device suite's cases reach."""
import importlib.util
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

from buildingsegment_amd import _lib, api

from test_simplify_cpu import twin_identity  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["bs_clean_outlines_count_dev", "bs_clean_outlines_emit_dev", "bs_clean_outlines", "bs_clean_outlines_free",
       "bs_clean_outlines_write_obj"]


def load_uncross_cases():
    if "uncross_cases" not in sys.modules:
        spec = importlib.util.spec_from_file_location("uncross_cases", os.path.join(HERE, "uncross_ref", "cases.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["uncross_cases"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["uncross_cases"]


cases = load_uncross_cases()
uref, brute = cases.uref, cases.brute
NAMED = dict(cases.named_cases())
_REF = {}


def ref(name, tol, max_rounds=-1, cell_log2=0):
    """(plain, simple, clean) of the restatement, computed once and never changed"""
    key = (name, tol, max_rounds, cell_log2)
    if key not in _REF:
        c = NAMED[name]
        _REF[key] = uref.clean(c["label"], c["top"], c["n_labels"], *tol, max_rounds=max_rounds, cell_log2=cell_log2)
    return _REF[key]


def segments_of(plain, s):
    out = []
    for r in range(plain.n_rings):
        a, b = int(s.s_ring_offset[r]), int(s.s_ring_offset[r + 1])
        for v in range(a, b):
            u = v + 1 if v + 1 < b else a
            out.append(((int(s.sxy[v, 0]), int(s.sxy[v, 1])), (int(s.sxy[u, 0]), int(s.sxy[u, 1])), int(plain.ring_label[r]),
                        int(s.s_right[v]), v))
    return out


def marked_by_all_pairs(plain, s):
    """an all-pairs test of its own: the common points of two closed segments A + u (B - A) and C + v (D - C) from the
    parameters u = un / den and v = vn / den as integers; a pair meets badly iff some common point is not an end point of
    both.  Returns the first vertices of the segments that meet another badly.  (Pairs whose boxes are apart are not
    evaluated: closed segments whose boxes are apart have no common point.)"""
    segs = segments_of(plain, s)
    if not segs:
        return set()
    e = np.array([[a[0], a[1], b[0], b[1], l, r] for a, b, l, r, _ in segs], np.int64)
    first = np.array([g[4] for g in segs])
    x0, x1, y0, y1 = np.minimum(e[:, 0], e[:, 2]), np.maximum(e[:, 0], e[:, 2]), np.minimum(e[:, 1], e[:, 3]), np.maximum(e[:, 1], e[:, 3])
    I, J = [], []
    order = np.argsort(x0, kind="stable")  # a sweep along X: j can meet i only while x0[j] <= x1[i]
    xs0, xs1, ys0, ys1 = x0[order], x1[order], y0[order], y1[order]
    ends = np.searchsorted(xs0, xs1, "right")
    for i in range(len(segs)):
        j = np.arange(i + 1, ends[i])
        j = j[(ys0[j] <= ys1[i]) & (ys1[j] >= ys0[i])]
        I.append(np.full(len(j), order[i]))
        J.append(order[j])
    I, J = np.concatenate(I), np.concatenate(J)
    a, c = e[I], e[J]
    twin = (a[:, 0] == c[:, 2]) & (a[:, 1] == c[:, 3]) & (a[:, 2] == c[:, 0]) & (a[:, 3] == c[:, 1]) & (a[:, 4] == c[:, 5]) & (a[:, 5] == c[:, 4])
    rx, ry, sx, sy = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], c[:, 2] - c[:, 0], c[:, 3] - c[:, 1]
    qx, qy = c[:, 0] - a[:, 0], c[:, 1] - a[:, 1]
    den, un, vn = rx * sy - ry * sx, qx * sy - qy * sx, qx * ry - qy * rx
    sg = np.where(den < 0, -1, 1)
    den, un, vn = den * sg, un * sg, vn * sg
    end_u, end_v = (un == 0) | (un == den), (vn == 0) | (vn == den)
    crossing = (den != 0) & (un >= 0) & (un <= den) & (vn >= 0) & (vn <= den) & ~(end_u & end_v)
    rr, t0 = rx * rx + ry * ry, qx * rx + qy * ry  # collinear: C and D along A -> B in units of 1 / |B - A|^2
    t1 = t0 + sx * rx + sy * ry
    overlap = (den == 0) & (vn == 0) & (np.maximum(np.minimum(t0, t1), 0) < np.minimum(np.maximum(t0, t1), rr))
    bad = ~twin & (crossing | overlap)
    return set(first[I[bad]].tolist()) | set(first[J[bad]].tolist())


def test_symbols_and_python_names():
    """fails before this stage existed: the header, the loader and the library name the new entry points"""
    txt = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert re.search(r"^struct bs_clean_outlines \{", txt, flags=re.M)
    L = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, txt) and name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("clean_outlines", "clean_outlines_dev", "clean_outlines_emit_dev"):
        assert hasattr(api.Context, name), name
    assert hasattr(api, "CleanOutlines") and hasattr(api, "write_clean_outlines_obj")
    assert L.bs_api_version() == 5


SMALL = sorted(n for n, c in NAMED.items() if c["label"].size <= 400)
MULTI_ROUND = sorted(cases.own_shapes())  # the only cases with more than one repair round
AGREE = SMALL + MULTI_ROUND + ["noisy_diagonal", "spiral"]


@pytest.mark.parametrize("name", AGREE)
def test_references_agree(name):
    """the restatement against the definition, at every cell size; the multi-round cases also under caps of 0, 1 and 2"""
    c = NAMED[name]
    for tol in cases.TOLERANCES:
        for cap in ((-1, 0, 1, 2) if name in MULTI_ROUND else (-1,)):
            _, b = brute.clean(c["label"], c["top"], c["n_labels"], *tol, max_rounds=cap)
            for k in (0,) + cases.CELL_LOG2:
                _, _, a = ref(name, tol, max_rounds=cap, cell_log2=k)
                assert uref.same(a, b) is None, (tol, cap, k, uref.same(a, b))


def test_conflicting_runs_are_the_known_ones():
    """of all named cases at all tolerances exactly these conflict"""
    got = {(n, t) for n in NAMED for t in cases.TOLERANCES if ref(n, t)[2].n_marked_first > 0}
    assert got == set(cases.CONFLICTING) | set(cases.CONFLICTING_FUZZ)
    assert all(ref(n, t)[2].repair_rounds == 1 for n, t in cases.CONFLICTING_FUZZ)
    for n, t in cases.CONFLICTING:
        assert ref(n, t)[2].repair_rounds == (3 if n in MULTI_ROUND else 1)
    f = ref("finger", (10 ** 6, 1))[2]
    assert (f.n_marked_first, f.repair_rounds, f.n_forced, f.n_marked_left) == (4, 3, 10, 0)
    assert (f.n_svertices_before, f.n_svertices, f.n_nodes) == (16, 26, 34)  # rings of 4 + 12 + 12 + 6 nodes


@pytest.mark.parametrize("name,tol", [("fuzz_1", (25, 4)), ("fuzz_2", (2, 1)), ("fuzz_10", (2, 1))])
def test_conflicting_fuzz_runs_agree_with_the_definition(name, tol):
    """the facet fuzz cases that conflict, at the lowest tolerance at which each does (thousands of segments: too slow for
    test_references_agree at every tolerance and cell size)"""
    c = NAMED[name]
    _, b = brute.clean(c["label"], c["top"], c["n_labels"], *tol)
    assert b.n_marked_first > 0 and uref.same(ref(name, tol)[2], b) is None


@pytest.mark.parametrize("name", sorted(NAMED))
def test_properties(name):
    for tol in cases.TOLERANCES:
        plain, simple, s = ref(name, tol)
        assert not marked_by_all_pairs(plain, s), tol  # no conflict is left
        assert s.n_marked_left == 0 and not (s.s_flag & 8).any()
        twin_identity(plain, s)
        assert (s.s_ring_vertices >= 3).all()
        _, nodes, _ = ref(name, (0, 1))
        for r in range(plain.n_rings):  # simplified kept set <= clean kept set <= nodes, as (ring, corner) sets
            rows = lambda o: Counter(map(tuple, o.sxy[int(o.s_ring_offset[r]):int(o.s_ring_offset[r + 1])].tolist()))  # noqa: E731
            assert not rows(simple) - rows(s) and not rows(s) - rows(nodes)
        assert (s.s_flag & 4 > 0).sum() == s.n_forced == s.n_svertices - simple.n_svertices
        _, _, chk = ref(name, tol, max_rounds=0)  # check only: the simplified result, bit 3 exactly on the marked segments
        assert np.array_equal(chk.sxy, simple.sxy) and np.array_equal(chk.s_flag & 3, simple.s_flag)
        # (without a conflict the check-only result has the geometry of s, which the all-pairs test above cleared)
        still = marked_by_all_pairs(plain, chk) if s.n_marked_first else set()
        assert (chk.n_marked_first > 0) == (s.n_marked_first > 0) and set(np.nonzero(chk.s_flag & 8)[0].tolist()) == still
        assert chk.n_marked_first == chk.n_marked_left == int((chk.s_flag & 8 > 0).sum()) and chk.repair_rounds == 0


def test_cap_of_one_round_on_finger():
    _, _, s = ref("finger", (10 ** 6, 1), max_rounds=1)
    assert s.repair_rounds == 1 and s.n_marked_left > 0 and (s.s_flag & 8 > 0).sum() == s.n_marked_left


def test_cases_reach_every_regime():
    seen = Counter()
    for name, tol in cases.CONFLICTING + (("rectangle", (10 ** 6, 1)), ("side_by_side", (10 ** 6, 1))):
        seen.update(cases.regimes(NAMED[name], tol))
    seen.update(cases.regimes(cases.sc.thin_u(), (cases.BIG_DEN, cases.BIG_DEN), 1))
    missing = [k for k in cases.REGIMES if seen[k] == 0]
    assert not missing, missing
    assert "cross" in cases.regimes(NAMED["random_20"], (25, 4)) and "touch" in cases.regimes(NAMED["random_30"], (10 ** 6, 1))
    assert "overlap_at_shared_end" in cases.regimes(NAMED["random_52"], (10 ** 6, 1))
    assert "twin_pair" in cases.regimes(NAMED["side_by_side"], (10 ** 6, 1))
