"""The references of the roof generalisation (include/bs_api.h, "roof generalisation") against each other, without a GPU:
the plain-Python definition (tests/generalise_ref/brute.py) against the numpy restatement (generalise_ref.py), the
identities every result satisfies, and the regimes the cases of the device suite reach."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def load_generalise_cases():
    """tests/generalise_ref/cases.py under a name of its own (other reference directories have a cases.py too)"""
    return _load("generalise_cases", os.path.join(HERE, "generalise_ref", "cases.py"))


cases = load_generalise_cases()
gr, fr, sr = cases.gr, cases.fr, cases.sr
SHAPES = cases.named_shapes()
NEW = ["bs_roof_generalise_dev", "bs_roof_generalise", "bs_roof_generalise_free"]


def identities(c, r):
    """what every result satisfies, from the inputs, the result and the facet reference alone"""
    bmap, roof0 = c["bmap"], c["roof"]
    inb = bmap >= 0
    p = c["params"]
    assert r.plane_pixels_in.sum() == r.plane_pixels_out.sum() == inb.sum()
    assert np.array_equal(r.roof[~inb], roof0[~inb])
    changed = r.roof != roof0
    assert r.pixels_changed == changed.sum() == r.building_pixels_changed.sum()
    assert (r.roof[changed] > 0).all()  # a pixel only ever changes to a plane
    assert r.pixels_roofed == ((roof0 <= 0) & (r.roof > 0) & inb).sum()
    n = r.rounds + 1
    assert all(len(getattr(r, k)) == n for k in gr.brute.EVAL)
    assert (r.eval_movers == r.eval_movers_small + r.eval_movers_flat).all()
    assert (r.eval_movers[:-1] > 0).all() and (r.eval_longest_chain[:-1] >= 1).all()
    assert (r.eval_facets[1:] <= r.eval_facets[:-1] - r.eval_movers[:-1]).all()
    assert r.converged == (r.eval_movers[-1] == 0) and r.rounds <= p["max_rounds"]
    assert (r.eval_longest_chain[-1] == 0) == (r.eval_movers[-1] == 0)
    if not p["merge_flat"]:
        assert r.eval_movers_flat.sum() == 0
    if p["min_pixels"] <= 1 and not p["merge_flat"]:
        assert r.rounds == 0 and np.array_equal(r.roof, roof0)
    if r.rounds == 0:
        assert np.array_equal(r.roof, roof0) and r.building_sum_abs_dtop.sum() == 0
    tabs = [c[k] for k in ("normal", "center", "z_min", "z_max", "bin", "base_z", "flat")]
    for tag, img in (("in", roof0), ("out", r.roof)):
        f = fr.roof_facets(bmap, img, sr.tops(bmap, img, *tabs))
        assert getattr(r, "n_facets_" + tag) == f.n_facets and getattr(r, "n_edges_" + tag) == f.n_edges
        assert getattr(r, "n_flat_" + tag) == (fr.kinds(f, p["step_tol"], p["bend_tol"]) == 0).sum()
        assert getattr(r, "n_small_" + tag) == (f.facet_pixels < p["min_pixels"]).sum()
        assert np.array_equal(getattr(r, "building_facets_" + tag), np.bincount(f.facet_building, minlength=c["n_buildings"]))
        assert np.array_equal(getattr(r, "plane_pixels_" + tag),
                              np.bincount(np.maximum(img[inb], 0), minlength=len(c["z_min"]) + 1))
    assert r.n_facets_in == r.eval_facets[0] and r.n_facets_out == r.eval_facets[-1]
    assert (r.building_max_abs_dtop <= r.building_sum_abs_dtop).all() and (r.building_max_abs_dtop >= 0).all()


def idempotent(c, r, run):
    """a converged output run again with the same parameters returns itself with rounds == 0"""
    if not r.converged:
        return
    again = dict(c)
    again["roof"] = r.roof
    r2 = run(again)
    assert r2.rounds == 0 and r2.converged == 1 and np.array_equal(r2.roof, r.roof)
    assert (r2.n_facets_in, r2.n_edges_in, r2.n_flat_in) == (r.n_facets_out, r.n_edges_out, r.n_flat_out)


@pytest.mark.parametrize("seed", range(cases.N_SMALL))
def test_brute_equals_restatement(seed):
    c = cases.small_case(seed)
    assert max(c["bmap"].shape) <= 12
    a, b = cases.run_brute(c), cases.run_ref(c)
    assert gr.same(a, b) is None, gr.same(a, b)
    identities(c, b)
    idempotent(c, b, cases.run_ref)


@pytest.mark.parametrize("name", sorted(n for n in SHAPES if n != "strip_4097"))
def test_named_shape_brute(name):
    c = SHAPES[name]
    a, b = cases.run_brute(c), cases.run_ref(c)
    assert gr.same(a, b) is None, gr.same(a, b)
    identities(c, b)
    idempotent(c, b, cases.run_ref)


@pytest.mark.parametrize("seed", range(cases.N_FUZZ))
def test_fuzz_identities(seed):
    c = cases.fuzz_case(seed)
    r = cases.run_ref(c)
    identities(c, r)
    idempotent(c, r, cases.run_ref)


def test_named_shapes_do_what_they_are_named_for():
    r = {k: cases.run_ref(c) for k, c in SHAPES.items()}
    for k in ("one_pixel", "one_facet", "small_beside_unroofed_only", "two_buildings_same_plane", "two_buildings_other_planes",
              "diagonal_only", "coplanar_without_merge_flat", "gable_is_a_ridge", "step"):
        assert r[k].rounds == 0 and r[k].converged == 1 and np.array_equal(r[k].roof, SHAPES[k]["roof"]), k
    assert r["island"].roof.tolist() == [[1] * 5] * 5 and r["island"].pixels_roofed == 0
    for k, other in (("unroofed_island_0", -1), ("unroofed_island_m1", 0)):
        assert r[k].pixels_roofed == 1 and r[k].roof[2, 2] == 1 and r[k].roof[0, :2].tolist() == [other, other], k
    assert r["length_tie_equal_pixels"].roof[2, 2] == 1  # north, west and south have two pixels: the lowest id, north
    assert r["length_tie_most_pixels"].roof[2, 2] == 3   # east has three
    assert r["two_small_facets"].roof.tolist() == [[1, 1, 1]] and r["two_small_facets"].eval_movers.tolist() == [1, 0]
    assert r["coplanar_merge_flat"].roof.tolist() == [[1] * 4] * 2 and r["coplanar_merge_flat"].eval_movers_flat.tolist() == [1, 0]
    assert fr.kinds(r["gable_is_a_ridge"].evals[0].rf, 200, 0).tolist() == [1]
    assert fr.kinds(r["step"].evals[0].rf, 200, 0).tolist() == [3]
    for n in (65, 257, 4097):
        s = r[f"strip_{n}"]
        assert s.eval_longest_chain.tolist() == [n - 1, 0] and s.rounds == 1 and (s.roof == 1).all()
    assert bin(4097 - 1).count("1") == 1 and (4097 - 1).bit_length() == 13  # 13 doubling rounds on the device
    cb = r["checkerboard_8"]
    assert cb.rounds == 1 and (cb.roof == 1).all() and cb.eval_longest_chain[0] == 14


def test_searched_seeds():
    c = cases.fuzz_case(cases.SEED_WAITS)
    assert "waits_then_moves" in cases.regimes(c) and cases.run_ref(c).rounds >= 2
    c = cases.fuzz_case(cases.SEED_THREE_ROUNDS)
    assert cases.run_ref(c).rounds >= 3
    capped = cases.run_ref(cases.with_params(c, max_rounds=1))
    assert capped.rounds == 1 and capped.converged == 0
    c = cases.fuzz_case(cases.SEED_FLAT_LATER)
    assert "flat_only_later" in cases.regimes(c)


def test_cases_reach_every_regime():
    seen = set()
    for _, c in cases.all_cases():
        seen |= cases.regimes(c)
    assert not set(cases.REGIMES) - seen, sorted(set(cases.REGIMES) - seen)


def test_header_loader_and_sources_name_the_stage():
    from buildingsegment_amd import _lib, build
    assert all(n in _lib.EXPORTS for n in NEW)
    assert "bs_generalise.hip" in build.SOURCES
    hdr = open(os.path.join(HERE, "..", "include", "bs_api.h")).read()
    assert f"#define BS_GEN_FIG_CAP {cases.FIG_CAP} " in hdr and f"#define BS_GEN_PLANE_CAP {cases.PLANE_CAP} " in hdr
    assert (_lib.GEN_FIG_CAP, _lib.GEN_PLANE_CAP) == (cases.FIG_CAP, cases.PLANE_CAP)
