"""The premises of tests/shard_ref/scenarios.py, checked without a GPU.  Every scenario exists to reach one branch of
bs_segment_sharded's orchestration; whether it does depends on facts about its cloud.  They are asserted here from the
CPU oracle's k-lists and scipy's connected components, and tests/test_gpu_sharded_scenarios.py then compares the
figures of bs_shard_info with the same computed numbers."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "shard_ref"))
import scenarios as S  # noqa: E402

IDS = [sc.name for sc in S.SCENARIOS]


@pytest.mark.parametrize("sc", S.SCENARIOS, ids=IDS)
def test_cloud_and_shares(sc):
    xyz = S.cloud(sc)
    n = len(xyz)
    assert xyz.dtype == np.int32 and xyz.shape == (n, 3) and 40 <= n <= 15000
    assert np.abs(xyz.astype(np.int64)).max() < (1 << 23)  # the exact domain of stages 1-2
    assert n >= sc.k and sc.world in (2, 3, 4)
    parts = S.shares(sc.rule, n, sc.world)
    assert len(parts) == sc.world and all(p.dtype == np.int32 for p in parts)
    assert np.array_equal(np.sort(np.concatenate(parts)), np.arange(n))  # a permutation of 0..n-1
    if sc.rule == "rank1_nothing":
        assert len(parts[1]) == 0 and all(len(p) > 0 for r, p in enumerate(parts) if r != 1)
    if sc.rule == "rank0_everything":
        assert len(parts[0]) == n
    if sc.rule in ("interleaved", "random"):  # no rank holds an index range
        assert all(len(p) > 1 and not np.array_equal(p, np.arange(p[0], p[0] + len(p))) for p in parts)


@pytest.mark.parametrize("sc", S.SCENARIOS, ids=IDS)
def test_components_retries_and_shift(oracle, sc):
    f = S.facts(oracle, sc)
    assert f["components"] == sc.components
    assert f["h0"] == (sc.halo if sc.halo >= S.RADIUS else (200.0 if sc.halo == 0 else S.RADIUS))
    # strict against non-strict comparison with h must not decide the count
    assert S.retry_margin(f["max_kth"], f["h0"]) > 1.0, f["max_kth"]
    assert f["retries"] == sc.retries, f["max_kth"]
    if sc.retries is None:
        assert f["max_kth"] > 64 * f["h0"] and f["labels"] is None
    else:
        assert f["halo_mm"] == f["h0"] * 2 ** sc.retries and f["max_kth"] < f["halo_mm"]
        assert sc.retries == 0 or f["max_kth"] > f["halo_mm"] / 2
        assert len(f["labels"]) == len(f["xyz"])
    assert S.expected_shift(f["xyz"]) == sc.shift


def test_expected_figures_of_the_named_cases(oracle):
    """The figures the scenarios were designed around."""
    f = S.facts(oracle, S.BY_NAME["disc_retry1_w3"])
    assert f["h0"] == 100.0 and 111.0 < np.median(f["kth"]) < 112.0 and 150.0 < f["max_kth"] < 160.0
    f = S.facts(oracle, S.BY_NAME["disc_lattice_retry4_w2"])
    assert 890.0 < f["max_kth"] < 900.0  # 400 * sqrt(5): a corner of the lattice block
    f = S.facts(oracle, S.BY_NAME["coarse_lattice_uncertified_w2"])
    assert f["max_kth"] > 6400.0
    # at least one multi-component scenario commits planes on more than one component, and the single-component ones
    # commit at least one (a rank that grew nothing is told apart from a rank whose planes were lost)
    for name in ("boxes3_contiguous_w2", "boxes6_random_w4", "far_boxes_w2", "walls_6k_w4", "disc_retry1_w3", "lattice24_ties_w3"):
        f = S.facts(oracle, S.BY_NAME[name])
        pl = f["planes"]
        assert len(pl["id"]) >= 1
        seeds = pl["point_idx"][pl["offset"][:-1]]
        if S.BY_NAME[name].components > 1:
            assert len(set(f["comp"][seeds].tolist())) > 1


def test_shift_decides_which_rank_grows_which_box(oracle):
    """Without the shift the keys of the far boxes are cut to 21 bits and the two boxes change places in the Morton
    order: the restated partition with shift 0 deals every box to the other rank."""
    sc = S.BY_NAME["far_boxes_w2"]
    f = S.facts(oracle, sc)
    xyz = f["xyz"]
    parts = S.shares(sc.rule, len(xyz), sc.world)
    good = S.expected_deal(f["comp"], S.expected_slabs(xyz, parts))[0]
    org = xyz.astype(np.int64).min(0)
    cut = ((xyz.astype(np.int64) - org) & ((1 << 21) - 1)) + org  # what shift 0 makes of the coordinates
    assert S.expected_shift(cut) == 0
    bad = S.expected_deal(f["comp"], S.expected_slabs(cut.astype(np.int32), parts))[0]
    assert (good != bad).all()
    seeds = f["planes"]["point_idx"][f["planes"]["offset"][:-1]]
    assert len(seeds) >= 2 and len(set(good[seeds].tolist())) == 2  # both ranks hold planes: a swap shows in the fetch


def test_shift_variants():
    a, b, c = (S.cloud(S.BY_NAME[n]) for n in ("far_boxes_w2", "far_boxes_domain_edge_w3", "far_boxes_negative_w2"))
    ext = int((a.astype(np.int64).max(0) - a.min(0)).max())
    assert (1 << 21) <= ext < (1 << 22) and ext > 3_000_000
    assert b.max() == (1 << 23) - 2 and np.array_equal(b.astype(np.int64) - b.min(0), a.astype(np.int64) - a.min(0))
    assert c.min() == -((1 << 23) - 2) and c.max() < 0 and np.array_equal(c, -b)
    assert S.expected_shift(a) == S.expected_shift(b) == S.expected_shift(c) == 1
    assert S.expected_shift(S.cloud(S.BY_NAME["boxes6_random_w4"])) == 0


def test_tiny_cloud_cannot_fill_a_k_list_per_slab():
    sc = S.BY_NAME["tiny40_w3"]
    xyz = S.cloud(sc)
    assert len(xyz) == 40 and sc.world == 3 and sc.k == 16
    x = np.sort(xyz[:, 0])
    patch = np.searchsorted([1000, 2400], xyz[:, 0])  # three patches along x
    assert np.bincount(patch).tolist() == [13, 12, 15] and max(np.bincount(patch)) < sc.k
    # more than two voxels of the smallest edge (500 mm) between the patches: the first exchanges bring nothing across
    assert np.diff(x).min() >= 0 and np.diff(x).max() >= 1100 and (np.diff(x) > 1000).sum() == 2
    # the partition of sharded_impl, restated: the slabs are the patches, so on every rank slab + halo stays below k
    # while the voxels are smaller than the gap -- only the branch for a slab that cannot fill a k-list asks for more
    slabs = S.expected_slabs(xyz, S.shares(sc.rule, 40, sc.world))
    assert all(0 < len(s) < sc.k for s in slabs) and sum(len(s) for s in slabs) == 40
    assert all(len(set(patch[s].tolist())) == 1 for s in slabs)
    # ... and within reach of the doublings
    assert int((xyz.max(0) - xyz.min(0)).max()) < 64 * S.start_halo(sc.halo)


def test_lattice_rows_tie_at_the_kth_place(oracle):
    sc = S.BY_NAME["lattice24_ties_w3"]
    xyz = S.cloud(sc)
    ng, _ = oracle.knn_normals(xyz, k=sc.k + 1, want_normals=False)
    q = xyz.astype(np.int64)
    d = ((q[ng] - q[:, None, :]) ** 2).sum(2)
    tied = d[:, sc.k - 1] == d[:, sc.k]  # the k-th and the runner-up are equidistant
    assert tied.sum() > len(xyz) // 2
    # the tie is decided by the global index, and the shuffle makes that differ from the order inside a Morton slab:
    # the winner has the smaller index, but not always the smaller Morton-ish (x, y, z) position
    win, lose = ng[tied, sc.k - 1], ng[tied, sc.k]
    assert (win < lose).all()
    pos = np.lexsort((xyz[:, 0], xyz[:, 1], xyz[:, 2]))
    rank_of = np.empty(len(xyz), np.int64)
    rank_of[pos] = np.arange(len(xyz))
    assert (rank_of[win] > rank_of[lose]).any() and (rank_of[win] < rank_of[lose]).any()
    assert np.array_equal(ng[:, :sc.k], S.facts(oracle, sc)["neigh"])  # the k-list is a prefix of the (k+1)-list


@pytest.mark.parametrize("sc", S.SCENARIOS, ids=IDS)
def test_restated_partition_is_a_balanced_partition(sc):
    xyz = S.cloud(sc)
    n = len(xyz)
    slabs = S.expected_slabs(xyz, S.shares(sc.rule, n, sc.world))
    assert np.array_equal(np.sort(np.concatenate(slabs)), np.arange(n))
    assert max(len(s) for s in slabs) <= 1.25 * n / sc.world


def test_retry_rule_restated():
    assert S.expected_retries(99.0, 100.0) == 0 and S.expected_retries(100.0, 100.0) == 1
    assert S.expected_retries(6399.0, 100.0) == 6 and S.expected_retries(6400.0, 100.0) is None
    assert S.start_halo(0.0) == 200.0 and S.start_halo(50.0) == 100.0 and S.start_halo(250.0) == 250.0
