"""tests/tools/fuzz_stages.py without a GPU: the case sequence is reproducible, the cases that the GPU test runs reach
every regime the fuzzer is there for (asserted on the references alone), and the references agree with independent
formulations of the same stages on the fuzz inputs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
sys.path.insert(0, os.path.join(HERE, "footprint_ref"))
sys.path.insert(0, os.path.join(HERE, "building_ref"))
import building_ref as bref  # noqa: E402
import fuzz_stages as F  # noqa: E402
import ref  # noqa: E402
from test_footprints_cpu import _scipy_close  # noqa: E402
from test_gpu_footprints import _external_components  # noqa: E402

SEED, CASES = F.GPU_TEST_SEED, F.GPU_TEST_CASES
MIN_CASES = 3  # every regime is reached in at least this many cases of the run


def _same_case(a, b):
    (ca, pa), (cb, pb) = a, b
    key = "xyz" if ca["kind"] == "cloud" else "ch1"
    return (ca["kind"], ca["sub"]) == (cb["kind"], cb["sub"]) and pa == pb and \
        ca[key].dtype == cb[key].dtype and np.array_equal(ca[key], cb[key], equal_nan=True)


def _generate(seed, cases):
    rng = np.random.default_rng(seed)
    return [F.build_case(F._sub_seed(rng)) for _ in range(cases)]


@pytest.fixture(scope="module")
def run(oracle):
    hit, built, per_case = F.coverage(SEED, CASES)
    return hit, built, per_case


def test_two_generations_are_identical_and_replay_reaches_every_case(run):
    _, built, _ = run
    again = _generate(SEED, CASES)
    assert len(again) == len(built) == CASES
    for a, b in zip(built, again):
        assert _same_case(a, b)
    for i in (0, 1, CASES // 2, CASES - 1):
        assert _same_case(F.replay_case(SEED, i), built[i])
    assert not _same_case(F.replay_case(SEED + 1, 0), built[0])


def test_cases_stay_inside_the_documented_domains(run):
    _, built, _ = run
    for case, p in built:
        assert p["kernel_size"] % 2 == 1 and 1 <= p["kernel_size"] <= 15
        assert 0 <= p["iterations"] <= 16 and 0 <= p["threshold"] <= 255
        if case["kind"] == "image":
            h, w = case["ch1"].shape
            assert case["ch1"].dtype == np.float64 and 1 <= h <= F.MAX_IMAGE[0] and 1 <= w <= F.MAX_IMAGE[1]
            continue
        xyz = F.ordered_cloud(case, p)
        ext = np.asarray(p["extent"])
        assert xyz.dtype == np.int32 and 1 <= len(xyz) < 2**29 and p["bin"] >= 1 and p["bin_height"] >= 1
        assert (xyz >= 0).all() and (xyz <= ext).all() and (ext < 2**31).all()  # raster domain; inside the map as well
        assert (ext[0] // p["bin"] + 2) * (ext[1] // p["bin"] + 2) <= F.MAX_PIXELS
        if not p["tail"]:  # an order of the same points
            assert np.array_equal(xyz[np.lexsort(xyz.T)], case["xyz"][np.lexsort(case["xyz"].T)])
        z, th = F.extreme_heights(p, len(xyz))
        assert z.dtype == np.int32 and len(z) == len(xyz) and F.I32_MIN <= th <= F.I32_MAX


def test_the_gpu_run_reaches_every_regime(run):
    """Conditions, not measurements: seed and count are chosen so that they hold, and the count is the smallest."""
    hit, _, per_case = run
    assert set(hit) == set(F.REGIMES + F.VARIANTS)
    short = {r: hit[r] for r in F.REGIMES if hit[r] < MIN_CASES}
    assert not short, short  # every regime in at least three cases
    unseen = [v for v in F.VARIANTS if hit[v] < 1]
    assert not unseen, unseen  # every kind of cloud and image, point order and second threshold at least once
    assert F.missing(hit) == []
    # If a change to the generator makes this fail, the count is no longer the smallest: pick the pair again -- for a
    # range of seeds, add cases until F.missing(counts) is empty, take the seed that needs the fewest, and write the
    # pair into GPU_TEST_SEED, GPU_TEST_CASES (and the count into README.md and DESIGN.md).
    without_last = {r: hit[r] - (r in per_case[-1]) for r in hit}
    assert F.missing(without_last), "a smaller count reaches everything: lower GPU_TEST_CASES"


def _image_of(oracle, case, p):
    if case["kind"] == "image":
        return F.full_image(case["ch1"])
    return oracle.grid_picture(F.ordered_cloud(case, p), extent=p["extent"], bin=p["bin"], bin_height=p["bin_height"])[0]


def test_references_agree_with_independent_formulations(run, oracle):
    """ref.mask against the numpy line of save_image + threshold, ref.close against scipy, and the start pixels of
    bref.building_map against scipy's labelling of the external components -- on every fuzz input."""
    _, built, _ = run
    for i, (case, p) in enumerate(built):
        img = _image_of(oracle, case, p)
        m = ref.mask(img, p["threshold"])
        assert np.array_equal(m, (F.quantised(img[..., 1]) > p["threshold"]).astype(np.uint8)), i
        closed = ref.close(m, p["kernel_size"], p["iterations"])
        assert np.array_equal(closed.astype(bool), _scipy_close(m, p["kernel_size"], p["iterations"])), i
        _, fmask = ref.footprints(img, p["threshold"], p["kernel_size"], p["iterations"])
        assert np.array_equal(fmask, closed), i
        b = bref.building_map(closed)
        starts = _external_components(closed)
        assert [tuple(s) for s in b.start_xy.tolist()] == starts[::-1], i


def test_quantised_is_the_restatement_on_the_boundaries():
    """the numpy line itself, where it is easy to check by hand: v = max * j / 255 gives j or j - 1, never j + 1"""
    for mx in (255.0, 1.0, 27.43, 1e-300, 1e300):
        x = mx * np.arange(256) / 255.0
        q = F.quantised(np.concatenate([x, [mx]])[None, :])[0, :256]
        assert ((q == np.arange(256)) | (q == np.arange(256) - 1)).all() and q[255] == 255 and q[0] == 0
    ch = np.array([[np.nan, -1.0, -0.0, np.inf, -np.inf, 5e-324, 3.0]])
    assert F.quantised(ch).tolist() == [[0, 0, 0, 0, 0, 0, 0]]  # max = inf: every quotient is 0 or NaN
    ch[0, 3] = 1.0
    assert F.quantised(ch).tolist() == [[0, 0, 0, 85, 0, 0, 255]]


def test_oracle_raster_equals_the_reference_binary_on_fuzz_clouds(run, oracle):
    if oracle.ref_raster_path() is None:
        pytest.skip("oracle/_ref/ref_raster is not built here")
    _, built, _ = run
    done = 0
    for case, p in built:
        if case["kind"] != "cloud" or (p["bin"], p["bin_height"]) != (100, 1000):
            continue
        xyz = F.ordered_cloud(case, p)
        xyz = np.ascontiguousarray(xyz - xyz.min(0, keepdims=True))
        r = oracle.ref_grid_picture(xyz)
        img, th = oracle.grid_picture(xyz, libm_log=True)
        assert th == r["ground_th"] and np.array_equal(img, r["image"])
        done += 1
    assert done >= 1
